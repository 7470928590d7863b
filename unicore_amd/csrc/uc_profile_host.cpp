// uc_profile_host.cpp — `unicore profile` (rule UC-P): the host counter, the checks both counters share and the file level.
//   module body      /root/reference/src/modules/profile.rs:13-147  (profile, output_statistics_and_genes)
//   its caller       /root/reference/src/modules/profile.rs:149-172 (run: output directory, profile.chk, <db>.map)
//   messages         /root/reference/src/util/message.rs:4-22, /root/reference/src/envs/error_handler.rs:17-39
// The device counter is uc_profile.hip.  The reference iterates hash maps where it writes a gene file and its warnings; both orders are fixed
// here to ascending species name in bytes.
#include <sys/stat.h>

#include <algorithm>
#include <charconv>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "uc_files.h"
#include "uc_profile.h"

namespace uc {

uint64_t profile_validate(const ProfileArgs &a) {
    if (a.n_groups >= PROFILE_ID_LIMIT || a.n_genes >= PROFILE_ID_LIMIT || a.n_species >= PROFILE_ID_LIMIT)
        fail(UC_ERR_ARGS, "profile: %u groups, %u genes, %u species: each must stay below 2^24", a.n_groups, a.n_genes, a.n_species);
    auto need = [](const void *p, const char *what) { if (!p) fail(UC_ERR_ARGS, "profile: %s must not be NULL", what); };
    if (a.n_rows) { need(a.group, "group"); need(a.gene, "gene"); }
    if (a.n_genes) need(a.sp_off, "sp_off");
    if (a.n_groups) { need(a.single, "single"); need(a.multiple, "multiple"); need(a.core, "core"); }
    if (a.n_species) need(a.full, "full");
    need(a.core_off, "core_off");
    // the gene -> species CSR: a set per gene, ascending
    if (a.n_genes) {
        if (a.sp_off[0] != 0) fail(UC_ERR_ARGS, "profile: sp_off[0] must be 0");
        for (uint32_t g = 0; g < a.n_genes; g++) {
            const uint64_t b = a.sp_off[g], e = a.sp_off[g + 1];
            if (e < b || e - b > a.n_species) fail(UC_ERR_ARGS, "profile: gene %u has a malformed species range", g);
            if (e > b) need(a.sp, "sp");
            for (uint64_t k = b; k < e; k++)
                if (a.sp[k] >= a.n_species || (k > b && a.sp[k] <= a.sp[k - 1]))
                    fail(UC_ERR_ARGS, "profile: the species of gene %u must be distinct, ascending and below %u", g, a.n_species);
        }
    }
    if ((a.n_rows == 0) != (a.n_groups == 0)) fail(UC_ERR_ARGS, "profile: %llu rows in %u groups", (unsigned long long)a.n_rows, a.n_groups);
    uint64_t pairs = 0;
    for (uint64_t i = 0; i < a.n_rows; i++) {
        const uint32_t g = a.group[i], prev = i ? a.group[i - 1] : 0;
        if (g < prev || g - prev > 1 || (i == 0 && g != 0))
            fail(UC_ERR_ARGS, "profile: group[%llu] = %u after %u: the group index starts at 0, never decreases and never skips", (unsigned long long)i, g, prev);
        const uint32_t x = a.gene[i];
        if (x == UC_NO_GENE) continue;
        if (x >= a.n_genes) fail(UC_ERR_ARGS, "profile: gene[%llu] = %u with %u genes", (unsigned long long)i, x, a.n_genes);
        pairs += a.sp_off[x + 1] - a.sp_off[x];
        if (pairs >> 32) fail(UC_ERR_ARGS, "profile: 2^32 or more (row, species) pairs");
    }
    if (a.n_rows && a.group[a.n_rows - 1] != a.n_groups - 1)
        fail(UC_ERR_ARGS, "profile: the last row is in group %u of %u", a.group[a.n_rows - 1], a.n_groups);
    if (pairs) { need(a.core_gene, "core_gene"); need(a.core_species, "core_species"); }
    return pairs;
}

void profile_count_host(const ProfileArgs &a, uint64_t) {
    const uint32_t S = a.n_species;
    const uint64_t thr_s = (uint64_t)a.threshold * S;
    std::vector<uint32_t> cnt(S, 0), first(S, 0), seen;
    std::vector<uint8_t> many(S, 0);      // a second distinct gene came in
    std::fill(a.full, a.full + S, 0u);
    uint64_t lines = 0, i = 0;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        seen.clear();
        for (; i < a.n_rows && a.group[i] == g; i++) {      // profile.rs:79-84
            const uint32_t x = a.gene[i];
            if (x == UC_NO_GENE) continue;
            for (uint64_t k = a.sp_off[x]; k < a.sp_off[x + 1]; k++) {
                const uint32_t s = a.sp[k];
                if (cnt[s]++ == 0) { seen.push_back(s); first[s] = x; }
                else if (first[s] != x) many[s] = 1;
            }
        }
        std::sort(seen.begin(), seen.end());
        uint32_t single = 0;
        for (uint32_t s : seen) single += cnt[s] == 1;      // profile.rs:121-122
        const bool core = (uint64_t)single * 100 >= thr_s;  // profile.rs:134
        a.single[g] = single; a.multiple[g] = (uint32_t)seen.size(); a.core[g] = core;
        a.core_off[g] = lines;
        for (uint32_t s : seen) {
            if (core) {
                if (cnt[s] == 1) a.full[s]++;                                                          // profile.rs:63-66
                if (!many[s]) { a.core_gene[lines] = first[s]; a.core_species[lines] = s; lines++; }   // profile.rs:138-143
            }
            cnt[s] = 0; many[s] = 0;
        }
    }
    a.core_off[a.n_groups] = lines;
}

namespace {

std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) fail(UC_ERR_IO, "cannot open %s", path.c_str());
    f.seekg(0, std::ios::end);
    const std::streamoff n = f.tellg();
    f.seekg(0);
    std::string s((size_t)std::max<std::streamoff>(n, 0), '\0');
    if (n > 0 && !f.read(&s[0], n)) fail(UC_ERR_IO, "cannot read %s", path.c_str());
    return s;
}

// the first two whitespace-separated fields of every line (profile.rs:21,51); a line with fewer is an error
template <typename F>
void two_fields(const std::string &text, const std::string &path, F &&row) {
    size_t p = 0, line = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        line++;
        std::string_view f[2];
        int k = 0;
        for (size_t q = p; q < e && k < 2;) {
            while (q < e && is_space(text[q])) q++;
            const size_t b = q;
            while (q < e && !is_space(text[q])) q++;
            if (q > b) f[k++] = std::string_view(text.data() + b, q - b);
        }
        if (k < 2) fail(UC_ERR_IO, "%s: line %zu has fewer than two fields", path.c_str(), line);
        row(f[0], f[1]);
        p = e + 1;
    }
}

// a double as Rust's `{}` prints it: the shortest decimal that round-trips, never an exponent, no ".0" behind a whole number
void append_percent(std::string &out, double x) {
    if (x != x) { out += "NaN"; return; }      // S == 0: an empty map
    char buf[512];
    const auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::fixed);
    out.append(buf, r.ptr);
}

bool host_counter_selected() {      // read per call, like the prefilter's switches
    const char *v = getenv("UC_PROFILE_HOST");
    return v && !strcmp(v, "1");
}

void profile_files(const char *db_prefix, const char *tsv, const char *out_dir, uint32_t threshold, const uc_opts *o) {
    if (threshold > 100) fail(UC_ERR_ARGS, "profile: threshold %u outside 0 .. 100", threshold);
    int verbosity = 3, device = -1;
    if (o) {
        if (o->struct_size != sizeof(uc_opts)) fail(UC_ERR_ARGS, "uc_opts.struct_size mismatch (%u != %zu)", o->struct_size, sizeof(uc_opts));
        verbosity = o->verbosity; device = o->device;
    }
    const bool timing = getenv("UC_TIMING") != nullptr;
    Timer t_all, t_part;
    double s_map = 0, s_tsv = 0, s_count = 0, s_write = 0;
    auto lap = [&](double &acc) { acc = t_part.seconds(); t_part = Timer(); };
    const std::string out = out_dir;
    make_dirs(out);
    write_file(out + "/profile.chk", "0");      // profile.rs:163

    // ---- the map (profile.rs:18-29): gene -> set of species; species ids by name in byte order
    const std::string map_path = std::string(db_prefix) + ".map";
    const std::string map_text = slurp(map_path);
    std::vector<std::string_view> gene_name, species_name;
    std::unordered_map<std::string_view, uint32_t> gene_id, species_id;
    std::vector<std::pair<uint32_t, std::string_view>> links;      // (gene id, species name)
    two_fields(map_text, map_path, [&](std::string_view g, std::string_view s) {
        const auto it = gene_id.emplace(g, (uint32_t)gene_name.size());
        if (it.second) gene_name.push_back(g);
        if (species_id.emplace(s, 0u).second) species_name.push_back(s);
        links.emplace_back(it.first->second, s);
    });
    std::sort(species_name.begin(), species_name.end());
    for (size_t k = 0; k < species_name.size(); k++) species_id[species_name[k]] = (uint32_t)k;
    if (gene_name.size() >= PROFILE_ID_LIMIT || species_name.size() >= PROFILE_ID_LIMIT)
        fail(UC_ERR_ARGS, "%s: %zu genes, %zu species: each must stay below 2^24", map_path.c_str(), gene_name.size(), species_name.size());
    const uint32_t n_genes = (uint32_t)gene_name.size(), S = (uint32_t)species_name.size();
    std::vector<uint64_t> link_key(links.size());
    for (size_t k = 0; k < links.size(); k++) link_key[k] = ((uint64_t)links[k].first << 32) | species_id[links[k].second];
    std::sort(link_key.begin(), link_key.end());
    link_key.erase(std::unique(link_key.begin(), link_key.end()), link_key.end());
    std::vector<uint64_t> sp_off((size_t)n_genes + 1, 0);
    std::vector<uint32_t> sp(link_key.size());
    for (size_t k = 0; k < link_key.size(); k++) { sp_off[(link_key[k] >> 32) + 1]++; sp[k] = (uint32_t)link_key[k]; }
    for (uint32_t g = 0; g < n_genes; g++) sp_off[g + 1] += sp_off[g];
    lap(s_map);

    // ---- the rows (profile.rs:50-77): a group is a maximal run of rows with the same first field
    const std::string tsv_text = slurp(tsv);
    std::vector<std::string_view> group_name;
    std::vector<uint32_t> group, gene;
    two_fields(tsv_text, tsv, [&](std::string_view q, std::string_view t) {
        if (group_name.empty() || group_name.back() != q) {
            if (group_name.size() + 1 >= PROFILE_ID_LIMIT) fail(UC_ERR_ARGS, "%s: 2^24 or more groups", tsv);
            group_name.push_back(q);
        }
        group.push_back((uint32_t)group_name.size() - 1);
        const auto it = gene_id.find(t);
        gene.push_back(it == gene_id.end() ? UC_NO_GENE : it->second);
    });
    const uint32_t n_groups = (uint32_t)group_name.size();
    lap(s_tsv);

    // ---- counting
    uint64_t cap = 0;
    for (uint32_t x : gene) if (x != UC_NO_GENE) cap += sp_off[x + 1] - sp_off[x];
    if (cap >> 32) fail(UC_ERR_ARGS, "profile: 2^32 or more (row, species) pairs");
    std::vector<uint32_t> single(n_groups), multiple(n_groups), full(S), core_gene(cap), core_species(cap);
    std::vector<uint8_t> core(n_groups);
    std::vector<uint64_t> core_off((size_t)n_groups + 1);
    ProfileArgs a{group.size(), group.data(), gene.data(), n_groups, n_genes, sp_off.data(), sp.data(), S, threshold,
                  single.data(), multiple.data(), core.data(), core_off.data(), core_gene.data(), core_species.data(), full.data()};
    const uint64_t n_pairs = profile_validate(a);
    const bool on_host = host_counter_selected();
    float ms[6] = {};
    if (verbosity >= 3) { fputs("Profiling the taxonomic distribution of the genes...", stdout); fflush(stdout); }      // profile.rs:49
    if (on_host) profile_count_host(a, n_pairs);
    else profile_count_device(device, a, n_pairs, timing ? ms : nullptr);
    lap(s_count);

    // ---- copiness.tsv and the gene files (profile.rs:120-147)
    std::string cop = "Query\tMultipleCopyPercent\tSingleCopyPercent\n", body;
    uint64_t n_core = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        const std::string_view name = group_name[g];
        const double sp_pct = (double)single[g] * 100.0 / (double)S, mp_pct = (double)multiple[g] * 100.0 / (double)S;
        if (verbosity >= 4) printf("Gene %.*s reported %.2f%% single copy and %.2f%% multiple copy\n", (int)name.size(), name.data(), sp_pct, mp_pct);   // profile.rs:128
        cop.append(name); cop += '\t'; append_percent(cop, mp_pct); cop += '\t'; append_percent(cop, sp_pct); cop += '\n';
        if (!core[g]) continue;
        n_core++;
        std::string_view stem = name;      // profile.rs:135: the second '-'-separated field, else the whole name
        const size_t d1 = name.find('-');
        if (d1 != std::string_view::npos) { const size_t d2 = name.find('-', d1 + 1); stem = name.substr(d1 + 1, d2 == std::string_view::npos ? d2 : d2 - d1 - 1); }
        body.clear();
        for (uint64_t k = core_off[g]; k < core_off[g + 1]; k++) {
            body.append(gene_name[core_gene[k]]); body += '\t'; body.append(species_name[core_species[k]]); body += '\n';
        }
        write_file(out + "/" + std::string(stem) + ".txt", body);
    }
    write_file(out + "/copiness.tsv", cop);
    if (verbosity >= 3) {      // profile.rs:106-107
        puts(" Done");
        printf("%llu structural core genes found from %u candidates\n", (unsigned long long)n_core, n_groups);
        fflush(stdout);
    }
    if (verbosity >= 2) {      // profile.rs:110-115
        const uint64_t half = (n_core + 1) / 2;
        for (uint32_t s = 0; s < S; s++)
            if (full[s] < half)
                fprintf(stderr, "Warning: Species %.*s has only %u core genes out of %llu core genes\n", (int)species_name[s].size(), species_name[s].data(), full[s],
                        (unsigned long long)n_core);
    }
    write_file(out + "/profile.chk", "1");      // profile.rs:169
    lap(s_write);
    if (timing)
        fprintf(stderr, "unicore-cluster[timing]: profile: %zu rows, %u groups, %u genes, %u species, %llu pairs (%s counter); map %.2f ms, tsv %.2f ms, count %.2f ms "
                        "(device: expand %.3f, sort %.3f, runs %.3f, groups %.3f, emit %.3f, sum %.3f ms), write %.2f ms, total %.2f ms\n",
                group.size(), n_groups, n_genes, S, (unsigned long long)n_pairs, on_host ? "host" : "device", s_map * 1e3, s_tsv * 1e3, s_count * 1e3,
                ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], s_write * 1e3, t_all.seconds() * 1e3);
}

ProfileArgs args_of(uint64_t n_rows, const uint32_t *group, const uint32_t *gene, uint32_t n_groups, uint32_t n_genes, const uint64_t *sp_off, const uint32_t *sp,
                    uint32_t n_species, uint32_t threshold, uint32_t *single, uint32_t *multiple, uint8_t *core, uint64_t *core_off, uint32_t *core_gene,
                    uint32_t *core_species, uint32_t *full) {
    return ProfileArgs{n_rows, group, gene, n_groups, n_genes, sp_off, sp, n_species, threshold, single, multiple, core, core_off, core_gene, core_species, full};
}

}  // namespace

}  // namespace uc

using namespace uc;

int uc_profile_count(uint64_t n_rows, const uint32_t *group, const uint32_t *gene, uint32_t n_groups, uint32_t n_genes, const uint64_t *sp_off,
                     const uint32_t *sp, uint32_t n_species, uint32_t threshold, uint32_t *single, uint32_t *multiple, uint8_t *core,
                     uint64_t *core_off, uint32_t *core_gene, uint32_t *core_species, uint32_t *full) {
    return guard([&] {
        const ProfileArgs a = args_of(n_rows, group, gene, n_groups, n_genes, sp_off, sp, n_species, threshold, single, multiple, core, core_off, core_gene, core_species, full);
        profile_count_host(a, profile_validate(a));
    });
}

int uc_profile_count_dev(int32_t device, uint64_t n_rows, const uint32_t *group, const uint32_t *gene, uint32_t n_groups, uint32_t n_genes,
                         const uint64_t *sp_off, const uint32_t *sp, uint32_t n_species, uint32_t threshold, uint32_t *single, uint32_t *multiple,
                         uint8_t *core, uint64_t *core_off, uint32_t *core_gene, uint32_t *core_species, uint32_t *full) {
    return guard([&] {
        const ProfileArgs a = args_of(n_rows, group, gene, n_groups, n_genes, sp_off, sp, n_species, threshold, single, multiple, core, core_off, core_gene, core_species, full);
        profile_count_device(device, a, profile_validate(a), nullptr);
    });
}

int uc_profile(const char *db_prefix, const char *tsv, const char *out_dir, uint32_t threshold, const uc_opts *o) {
    return guard([&] {
        if (!db_prefix || !tsv || !out_dir) fail(UC_ERR_ARGS, "profile: db_prefix, tsv and out_dir must not be NULL");
        profile_files(db_prefix, tsv, out_dir, threshold, o);
    });
}
