// unicore_main.cpp — C++ host mirror of the reference's `unicore cluster`, `unicore search`, `unicore profile`, `unicore tree` and `unicore gene-tree` module
// surfaces (the two tree modules with the built-in builder `nj`; the reference's builders are external programs).
// (The reference host is Rust; no Rust toolchain exists in this image — SURVEY.md 0.2/D3 — so the host
// above the C ABI is C++ with the same names, argument meaning and error behaviour.)
//   CLI surface      /root/reference/src/util/arg_parser.rs:225-246  (Commands::Cluster), :271-293 (Commands::Profile), :296-330 (Commands::Tree)
//   module body      /root/reference/src/modules/cluster.rs:9-84     (modules::cluster::run)
//   checkpoint       /root/reference/src/util/checkpoint.rs:2-5
//   error/exit codes /root/reference/src/envs/error_handler.rs:5-45
//   messages         /root/reference/src/util/message.rs:4-22
// The three `foldseek` spawns of cluster.rs:45-76 become three in-process calls through the C ABI.
#include <sys/stat.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <unistd.h>
#include <algorithm>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "unicore_cluster.h"

namespace {

constexpr int ERR_GENERAL = 0x01, ERR_ARGPARSE = 0x40;   // error_handler.rs:6,13
int g_verbosity = 3;                                       // variables.rs:146

void print_message(const std::string &m, int level) { if (level <= g_verbosity) { fputs(m.c_str(), stdout); fflush(stdout); } }
void println_message(const std::string &m, int level) { if (level <= g_verbosity) { puts(m.c_str()); } }
[[noreturn]] void error(int code, const std::string &object) {   // error_handler.rs:42-45
    if (1 <= g_verbosity) fprintf(stderr, "%s%s\n", code == ERR_ARGPARSE ? "Argument parsing error: " : "Error: ", object.c_str());
    exit(code);
}

void write_checkpoint(const std::string &file, const char *content) {   // checkpoint.rs:2-5 (no newline)
    std::ofstream f(file, std::ios::binary | std::ios::trunc);
    if (!f) error(ERR_GENERAL, "Could not write checkpoint " + file);
    f << content;
}

void create_dir_all(const std::string &path) {
    std::string cur;
    for (size_t i = 0; i <= path.size(); i++) {
        if ((i == path.size() || path[i] == '/') && !cur.empty() && cur != "/") {
            struct stat st;
            if (stat(cur.c_str(), &st) != 0 && mkdir(cur.c_str(), 0777) != 0) error(ERR_GENERAL, "Could not create directory " + cur);
        }
        if (i < path.size()) cur.push_back(path[i]);
    }
}

void usage(FILE *to) {
    fputs("Usage: unicore cluster [OPTIONS] <INPUT> <OUTPUT> <TMP>\n\n"
         "Arguments:\n"
         "  <INPUT>   Input database (createdb output)\n"
         "  <OUTPUT>  Output prefix; the result will be saved as OUTPUT.tsv\n"
         "  <TMP>     Temp directory\n\n"
         "Options:\n"
         "  -k, --keep-cluster-db            Keep intermediate cluster database\n"
         "  -c, --cluster-options <STRING>   Arguments for foldseek-style options in string e.g. -c \"-c 0.8\" [default: \"-c 0.8\"]\n"
         "      --threads <THREADS>          Number of threads to use; 0 to use all [default: 0]\n"
         "  -v, --verbosity <VERBOSITY>      Verbosity (0: quiet, 1: +errors, 2: +warnings, 3: +info, 4: +debug) [default: 3]\n"
         "  -h, --help                       Print help\n", to);
}

// modules::cluster::run (cluster.rs:9-84)
int cluster_run(const std::string &input, const std::string &output, const std::string &tmp, bool keep_cluster_db,
                const std::string &cluster_options, int threads) {
    const int engine_verbosity = g_verbosity == 4 ? 3 : g_verbosity == 3 ? 2 : g_verbosity;   // cluster.rs:18
    // parent directory of the output (cluster.rs:21-29).  Deviation: an OUTPUT without a directory
    // component yields "" in the reference (checkpoint lands in "/cluster.chk"); "." is the intent.
    size_t slash = output.find_last_of('/');
    std::string parent = slash == std::string::npos ? "." : (slash == 0 ? "/" : output.substr(0, slash));
    create_dir_all(parent);
    write_checkpoint(parent + "/cluster.chk", "0");   // cluster.rs:32

    const std::string output_cluster_db = output + "_cluster", output_tsv = output + ".tsv";   // cluster.rs:43-44
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.threads = threads;
    o.verbosity = engine_verbosity;
    o.device = -1;
    o.num_gpus = 0;   // all visible GPUs; "--gpus N" inside the option string narrows it
    o.cluster_options = cluster_options.c_str();

    print_message("Running cluster on the MI355X engine...", 3);   // cluster.rs:52
    if (g_verbosity >= 3) putchar('\n');
    int rc = uc_cluster(input.c_str(), output_cluster_db.c_str(), tmp.c_str(), &o, nullptr);   // cluster.rs:45-55
    if (rc != 0) error(ERR_GENERAL, std::string("cluster engine failed with code ") + std::to_string(rc) + "\n" + uc_last_error());   // command.rs:10-14
    println_message(" Done", 3);                                    // cluster.rs:56
    rc = uc_createtsv(input.c_str(), output_cluster_db.c_str(), output_tsv.c_str(), &o);           // cluster.rs:59-64
    if (rc != 0) error(ERR_GENERAL, std::string("createtsv failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    if (!keep_cluster_db) {                                         // cluster.rs:67-76
        rc = uc_rmdb(output_cluster_db.c_str());
        if (rc != 0) error(ERR_GENERAL, std::string("rmdb failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    }
    write_checkpoint(parent + "/cluster.chk", "1");   // cluster.rs:81
    return 0;
}

void usage_search(FILE *to) {
    fputs("Usage: unicore search [OPTIONS] <INPUT> <TARGET> <OUTPUT> <TMP>\n\n"
         "Arguments:\n"
         "  <INPUT>   Input database\n"
         "  <TARGET>  Target database to search against\n"
         "  <OUTPUT>  Output prefix; the result will be saved as OUTPUT.m8\n"
         "  <TMP>     Temp directory\n\n"
         "Options:\n"
         "  -k, --keep-aln-db                Keep intermediate Foldseek alignment database\n"
         "  -s, --search-options <STRING>    Arguments for foldseek-style options in string e.g. -s \"-c 0.8\" [default: \"-c 0.8\"]\n"
         "      --threads <THREADS>          Number of threads to use; 0 to use all [default: 0]\n"
         "  -v, --verbosity <VERBOSITY>      Verbosity (0: quiet, 1: +errors, 2: +warnings, 3: +info, 4: +debug) [default: 3]\n"
         "  -h, --help                       Print help\n", to);
}

// modules::search::run (search.rs:8-84)
int search_run(const std::string &input, const std::string &target, const std::string &output, const std::string &tmp, bool keep_aln_db,
               const std::string &search_options, int threads) {
    const int engine_verbosity = g_verbosity == 4 ? 3 : g_verbosity == 3 ? 2 : g_verbosity;
    size_t slash = output.find_last_of('/');
    std::string parent = slash == std::string::npos ? "." : (slash == 0 ? "/" : output.substr(0, slash));   // search.rs:21-29
    create_dir_all(parent);
    write_checkpoint(parent + "/search.chk", "0");   // search.rs:32
    const std::string output_aln_db = output + "_aln", output_m8 = output + ".m8";   // search.rs:43-44
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.threads = threads;
    o.verbosity = engine_verbosity;
    o.device = -1;
    o.num_gpus = 0;   // all visible GPUs; "--gpus N" inside the option string narrows it
    o.cluster_options = search_options.c_str();
    print_message("Running search on the MI355X engine...", 3);
    if (g_verbosity >= 3) putchar('\n');
    // search.rs:45-46 hands <TARGET> to `foldseek search` as the query DB and <INPUT> as the target DB; kept as is
    int rc = uc_search(target.c_str(), input.c_str(), output_aln_db.c_str(), tmp.c_str(), &o, nullptr);   // search.rs:45-55
    if (rc != 0) error(ERR_GENERAL, std::string("search engine failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    println_message(" Done", 3);
    uc_opts oc = o;
    oc.cluster_options = "";   // convertalis gets no options (search.rs:57-60): OUTPUT.m8 is the 12 default columns whatever the search options say
    rc = uc_convertalis(target.c_str(), input.c_str(), output_aln_db.c_str(), output_m8.c_str(), &oc);    // search.rs:57-63
    if (rc != 0) error(ERR_GENERAL, std::string("convertalis failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    if (!keep_aln_db) {                                                                                   // search.rs:66-75
        rc = uc_rmdb(output_aln_db.c_str());
        if (rc != 0) error(ERR_GENERAL, std::string("rmdb failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    }
    write_checkpoint(parent + "/search.chk", "1");   // search.rs:80
    return 0;
}

// clap's own failures (missing positional, unknown flag, bad value) print "error: ..." + a usage hint on stderr and exit
// with status 2; `arg_required_else_help = true` (arg_parser.rs:8,226) prints the HELP text — also status 2 — when the
// (sub)command gets no argument at all.  ERR_ARGPARSE (0x40) is reserved for cluster.rs:11-15's unwrap_or_else arms, which
// clap's required positionals make unreachable.
constexpr int CLAP_USAGE = 2;
[[noreturn]] void clap_error(bool is_search, const std::string &what) {
    fprintf(stderr, "error: %s\n\nUsage: unicore %s\n\nFor more information, try '--help'.\n", what.c_str(),
            is_search ? "search [OPTIONS] <INPUT> <TARGET> <OUTPUT> <TMP>" : "cluster [OPTIONS] <INPUT> <OUTPUT> <TMP>");
    exit(CLAP_USAGE);
}

void usage_profile(FILE *to) {
    fputs("Usage: unicore profile [OPTIONS] <INPUT_DB> <INPUT_TSV> <OUTPUT>\n\n"
         "Arguments:\n"
         "  <INPUT_DB>   Input database (createdb output)\n"
         "  <INPUT_TSV>  Input tsv file (cluster or search output)\n"
         "  <OUTPUT>     Output directory\n\n"
         "Options:\n"
         "  -t, --threshold <THRESHOLD>      Coverage threshold for core structures. [0 - 100] [default: 80]\n"
         "  -p, --print-copiness             Generate tsv with copy number statistics\n"
         "      --threads <THREADS>          Number of threads to use; 0 to use all [default: 0]\n"
         "  -v, --verbosity <VERBOSITY>      Verbosity (0: quiet, 1: +errors, 2: +warnings, 3: +info, 4: +debug) [default: 3]\n"
         "  -h, --help                       Print help\n", to);
}

[[noreturn]] void clap_error_profile(const std::string &what) {
    fprintf(stderr, "error: %s\n\nUsage: unicore profile [OPTIONS] <INPUT_DB> <INPUT_TSV> <OUTPUT>\n\nFor more information, try '--help'.\n", what.c_str());
    exit(CLAP_USAGE);
}

// Commands::Profile (arg_parser.rs:271-293) + modules::profile::run (profile.rs:149-172): the output directory, profile.chk, the messages and
// the warnings are uc_profile's, which takes Unicore's own verbosity scale
int profile_main(int argc, char **argv) {
    if (argc == 2) { usage_profile(stderr); return CLAP_USAGE; }   // arg_required_else_help
    std::vector<std::string> pos;
    uint32_t threshold = 80;      // arg_parser.rs:282
    int verbosity = 3;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto value = [&]() -> std::string {
            if (i + 1 >= argc) clap_error_profile("a value is required for '" + a + "' but none was supplied");
            return argv[++i];
        };
        auto parse_threshold = [&](const std::string &v) {   // threshold_in_range (arg_parser.rs:18-25)
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos)
                clap_error_profile("invalid value '" + v + "' for '--threshold <THRESHOLD>': Not a number");
            const long t = v.size() > 9 ? 101 : atol(v.c_str());
            if (t > 100) clap_error_profile("invalid value '" + v + "' for '--threshold <THRESHOLD>': Threshold `" + v + "` is not in range 0 to 100");
            threshold = (uint32_t)t;
        };
        if (a == "-t" || a == "--threshold") parse_threshold(value());
        else if (a.rfind("--threshold=", 0) == 0) parse_threshold(a.substr(12));
        else if (a == "-p" || a == "--print-copiness") {}   // always true (arg_parser.rs:285-286)
        else if (a == "--threads") (void)value();            // the module has no threaded part (profile.rs never reads it)
        else if (a == "-v" || a == "--verbosity") verbosity = atoi(value().c_str());
        else if (a == "-h" || a == "--help") { usage_profile(stdout); return 0; }
        else if (a.size() > 1 && a[0] == '-') clap_error_profile("unexpected argument '" + a + "' found");
        else pos.push_back(a);
    }
    if (pos.size() < 3) clap_error_profile("the following required arguments were not provided");
    if (pos.size() > 3) clap_error_profile("unexpected argument '" + pos[3] + "' found");
    if (verbosity < 0 || verbosity > 4) clap_error_profile("invalid value for '--verbosity <VERBOSITY>'");
    g_verbosity = verbosity;
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.threads = 1;
    o.verbosity = verbosity;
    o.device = -1;
    const int rc = uc_profile(pos[0].c_str(), pos[1].c_str(), pos[2].c_str(), threshold, &o);
    if (rc != 0) error(ERR_GENERAL, std::string("profile failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    return 0;
}

void usage_tree(FILE *to) {
    fputs("Usage: unicore tree [OPTIONS] <--no-inference|--tree-builder nj> <DB> <INPUT> <OUTPUT>\n\n"
         "Arguments:\n"
         "  <DB>      Input database (createdb output)\n"
         "  <INPUT>   Input directory containing core structures (profile output)\n"
         "  <OUTPUT>  Output directory\n\n"
         "Options:\n"
         "  -a, --aligner <ALIGNER>                  Multiple sequence aligner [star, profile]; profile refines the star alignment against its own column\n"
         "                                           profile; progressive merges the rows along a guide tree by profile-profile alignment and keeps every residue;\n"
         "                                           foldmason, mafft-linsi and mafft are external programs and are refused [default: star]\n"
         "      --refine-iters <N>                   Rounds of profile refinement of the profile aligner [1 - 8] [default: 1]\n"
         "  -t, --tree-builder <TREE_BUILDER>        Phylogenetic tree builder [nj, iqtree, fasttree, raxml-ng]; nj (neighbour joining, built in) writes\n"
         "                                           <OUTPUT>/nj.nwk; the others are external programs: parsed, not run [default: iqtree]\n"
         "  -o, --aligner-options <ALIGNER_OPTIONS>  Foldseek-style options for the gapped stage behind the star aligner, e.g. -o \"--gap-open 12\"\n"
         "  -n, --no-inference                       Stop the tree module after alignment (before tree inference); required unless the builder is nj\n"
         "  -p, --tree-options <TREE_OPTIONS>        Options for tree builder; nj: \"--model kimura|p\" [default: kimura], \"--bootstrap B\" replicates label\n"
         "                                           every internal branch with its support in percent [default: 0], \"--seed S\" of their draws\n"
         "                                           [default: 1], \"--support fbp|tbe\" the share of replicates with the same branch or the\n"
         "                                           transfer bootstrap expectation [default: fbp]; parsed, not used for the others\n"
         "  -d, --threshold <THRESHOLD>              Gap threshold for multiple sequence alignment [0 - 100] [default: 50]\n"
         "  -c, --threads <THREADS>                  Number of threads to use; 0 to use all [default: 0]\n"
         "  -v, --verbosity <VERBOSITY>              Verbosity (0: quiet, 1: +errors, 2: +warnings, 3: +info, 4: +debug) [default: 3]\n"
         "  -h, --help                               Print help\n", to);
}

[[noreturn]] void clap_error_tree(const std::string &what) {
    fprintf(stderr, "error: %s\n\nUsage: unicore tree [OPTIONS] --no-inference <DB> <INPUT> <OUTPUT>\n\nFor more information, try '--help'.\n", what.c_str());
    exit(CLAP_USAGE);
}

// the options of the built-in builder: "--model kimura|p", "--bootstrap B" (0 .. 100000), "--seed S" (64 bits) and "--support fbp|tbe", each also as
// --word=value; any other word is refused by name, a value that is no number in range or no name of a rule too
struct NjOptions { std::string model = "kimura"; uint32_t bootstrap = 0; uint64_t seed = 1; std::string support = "fbp"; };

uint64_t nj_number_of(const std::string &word, const std::string &v, uint64_t most) {
    bool ok = !v.empty() && v.size() <= 20 && v.find_first_not_of("0123456789") == std::string::npos;
    unsigned long long x = 0;
    if (ok) { errno = 0; x = strtoull(v.c_str(), nullptr, 10); ok = errno == 0 && x <= most; }
    if (!ok) error(ERR_GENERAL, "tree builder nj: '" + v + "' is not a value for " + word + " (a number from 0 to " + std::to_string(most) + ")");
    return x;
}

NjOptions nj_options_of(const std::string &tree_options) {
    std::vector<std::string> words;
    for (size_t p = 0; p < tree_options.size();) {
        while (p < tree_options.size() && isspace((unsigned char)tree_options[p])) p++;
        const size_t b = p;
        while (p < tree_options.size() && !isspace((unsigned char)tree_options[p])) p++;
        if (p > b) words.push_back(tree_options.substr(b, p - b));
    }
    NjOptions o;
    for (size_t k = 0; k < words.size(); k++) {
        auto value = [&](const char *name, const char *what, std::string &v) {      // --name V or --name=V
            const std::string eq = std::string(name) + "=";
            if (words[k] == name) {
                if (k + 1 >= words.size()) error(ERR_GENERAL, std::string("tree builder nj: ") + name + " needs a value (" + what + ")");
                v = words[++k];
                return true;
            }
            if (words[k].rfind(eq, 0) == 0) { v = words[k].substr(eq.size()); return true; }
            return false;
        };
        std::string v;
        if (value("--model", "kimura, p", v)) o.model = v;
        else if (value("--bootstrap", "replicates, 0 .. 100000", v)) o.bootstrap = (uint32_t)nj_number_of("--bootstrap", v, 100000);
        else if (value("--seed", "a 64-bit number", v)) o.seed = nj_number_of("--seed", v, UINT64_MAX);
        else if (value("--support", "fbp, tbe", v)) o.support = v;
        else error(ERR_GENERAL, "tree builder nj does not know the option '" + words[k] + "' (--model kimura|p, --bootstrap B, --seed S, --support fbp|tbe)");
    }
    if (o.support != "fbp" && o.support != "tbe") error(ERR_GENERAL, "tree builder nj: '" + o.support + "' is not a value for --support (fbp, tbe)");
    if (o.model != "kimura" && o.model != "p") error(ERR_GENERAL, "tree builder nj does not know the model '" + o.model + "' (kimura, p)");
    return o;
}

// the inference call of both modules: the plain entry point without --bootstrap, so that every byte written is what it wrote before the option existed
// (threads: -c, 0 = all; only the replicates' host side - transform, support - is spread over them)
int nj_infer(const std::string &msa, const std::string &out, const NjOptions &nj, const uc_opts &o, int threads) {
    if (!nj.bootstrap) return uc_tree_infer(msa.c_str(), out.c_str(), nj.model.c_str(), &o, nullptr);
    uc_opts ob = o;
    ob.threads = threads > 0 ? threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));      // n^2 logs a replicate: more do not pay
    if (nj.support == "tbe") return uc_tree_infer_support(msa.c_str(), out.c_str(), nj.model.c_str(), nj.bootstrap, nj.seed, UC_NJ_SUPPORT_TBE, &ob, nullptr);
    return uc_tree_infer_boot(msa.c_str(), out.c_str(), nj.model.c_str(), nj.bootstrap, nj.seed, &ob, nullptr);
}

[[noreturn]] void refuse_external_builder(const std::string &builder) {
    error(ERR_GENERAL, "tree inference would start the external program " + builder + ", which this build does not do; pass -n/--no-inference and run it on combined.fasta");
}

// Commands::Tree (arg_parser.rs:296-330) + modules::tree::run (tree.rs:17-161): files, tree.chk and messages up to the concatenation are uc_tree's, which
// takes Unicore's own verbosity scale.  The aligner is the built-in centre-star MSA and the one builder that runs is the built-in `nj` (uc_tree_infer);
// the reference's aligners and tree builders are external programs, which this host does not start.
int tree_main(int argc, char **argv) {
    std::vector<std::string> pos;
    std::string aligner = "star", builder = "iqtree", aligner_options, tree_options;
    bool no_inference = false, refine_given = false;
    uint32_t threshold = 50;      // arg_parser.rs:322
    uint32_t refine_iters = 1;    // of the profile aligner
    int verbosity = 3, threads = 0;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto value = [&]() -> std::string {
            if (i + 1 >= argc) clap_error_tree("a value is required for '" + a + "' but none was supplied");
            return argv[++i];
        };
        auto parse_threshold = [&](const std::string &v) {   // threshold_in_range (arg_parser.rs:18-25)
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos)
                clap_error_tree("invalid value '" + v + "' for '--threshold <THRESHOLD>': Not a number");
            const long t = v.size() > 9 ? 101 : atol(v.c_str());
            if (t > 100) clap_error_tree("invalid value '" + v + "' for '--threshold <THRESHOLD>': Threshold `" + v + "` is not in range 0 to 100");
            threshold = (uint32_t)t;
        };
        auto parse_refine = [&](const std::string &v) {
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos)
                clap_error_tree("invalid value '" + v + "' for '--refine-iters <N>': Not a number");
            const long n = v.size() > 9 ? 9 : atol(v.c_str());
            if (n < 1 || n > UC_TREE_MAX_REFINE) clap_error_tree("invalid value '" + v + "' for '--refine-iters <N>': `" + v + "` is not in range 1 to 8");
            refine_iters = (uint32_t)n; refine_given = true;
        };
        if (a == "-a" || a == "--aligner") aligner = value();
        else if (a.rfind("--aligner=", 0) == 0) aligner = a.substr(10);
        else if (a == "-t" || a == "--tree-builder") builder = value();
        else if (a.rfind("--tree-builder=", 0) == 0) builder = a.substr(15);
        else if (a == "-o" || a == "--aligner-options") aligner_options = value();
        else if (a.rfind("--aligner-options=", 0) == 0) aligner_options = a.substr(18);
        else if (a == "-p" || a == "--tree-options") tree_options = value();
        else if (a.rfind("--tree-options=", 0) == 0) tree_options = a.substr(15);
        else if (a == "-n" || a == "--no-inference") no_inference = true;
        else if (a == "--refine-iters") parse_refine(value());
        else if (a.rfind("--refine-iters=", 0) == 0) parse_refine(a.substr(15));
        else if (a == "-d" || a == "--threshold") parse_threshold(value());
        else if (a.rfind("--threshold=", 0) == 0) parse_threshold(a.substr(12));
        else if (a == "-c" || a == "--threads") threads = atoi(value().c_str());      // read by the bootstrap of nj alone
        else if (a == "-v" || a == "--verbosity") verbosity = atoi(value().c_str());
        else if (a == "-h" || a == "--help") { usage_tree(stdout); return 0; }
        else if (a.size() > 1 && a[0] == '-') clap_error_tree("unexpected argument '" + a + "' found");
        else pos.push_back(a);
    }
    if (pos.size() < 3) clap_error_tree("the following required arguments were not provided");
    if (pos.size() > 3) clap_error_tree("unexpected argument '" + pos[3] + "' found");
    if (verbosity < 0 || verbosity > 4) clap_error_tree("invalid value for '--verbosity <VERBOSITY>'");
    g_verbosity = verbosity;
    if (aligner == "foldmason" || aligner == "mafft" || aligner == "mafft-linsi")      // tree.rs:42-45: ERR_BINARY_NOT_FOUND in the reference
        error(ERR_GENERAL, "aligner " + aligner + " is an external program, which this build does not start; the built-in aligner is 'star'");
    const bool profile = aligner == "profile";
    const bool progressive = aligner == "progressive";
    if (aligner != "star" && !profile && !progressive) error(ERR_GENERAL, "Unrecognized aligner");      // tree.rs:118
    if (refine_given && !profile) error(ERR_GENERAL, "--refine-iters belongs to the aligner 'profile'; the aligner '" + aligner + "' has no rounds");
    const bool nj = builder == "nj";
    if (!nj && builder != "iqtree" && builder != "fasttree" && builder != "raxml-ng") error(ERR_GENERAL, "Unrecognized tree builder");   // tree.rs:146
    const NjOptions nj_opts = nj ? nj_options_of(tree_options) : NjOptions();
    if (!no_inference && !nj) refuse_external_builder(builder);
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.threads = 1;
    o.verbosity = verbosity;
    o.device = -1;
    int rc = progressive ? uc_tree_progressive(pos[0].c_str(), pos[1].c_str(), pos[2].c_str(), threshold, aligner_options.c_str(), &o, nullptr)
           : profile ? uc_tree_refined(pos[0].c_str(), pos[1].c_str(), pos[2].c_str(), threshold, aligner_options.c_str(), refine_iters, &o, nullptr)
                     : uc_tree(pos[0].c_str(), pos[1].c_str(), pos[2].c_str(), threshold, aligner_options.c_str(), &o, nullptr);
    if (rc != 0) error(ERR_GENERAL, std::string("tree failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    if (no_inference) return 0;      // tree.rs:135-137 skips the alignment when combined.fasta exists and infers all the same
    print_message("Inferring phylogenetic tree...", 3);      // tree.rs:150
    rc = nj_infer(pos[2] + "/combined.fasta", pos[2] + "/nj.nwk", nj_opts, o, threads);
    if (rc != 0) error(ERR_GENERAL, std::string("tree inference failed with code ") + std::to_string(rc) + "\n" + uc_last_error());
    println_message(" Done", 3);
    write_checkpoint(pos[2] + "/tree.chk", "1");             // tree.rs:161
    return 0;
}

void usage_gene_tree(FILE *to) {
    fputs("Usage: unicore gene-tree [OPTIONS] --tree-builder nj <INPUT>\n\n"
         "Arguments:\n"
         "  <INPUT>  Input directory containing species phylogenetic tree (Output of the Tree module)\n\n"
         "Options:\n"
         "  -n, --names <NAMES>                      File containing core structures for computing phylogenetic tree; all of them if not given\n"
         "  -t, -T, --tree-builder <TREE_BUILDER>    Phylogenetic tree builder [nj, iqtree, fasttree, raxml-ng]; nj (neighbour joining, built in) writes\n"
         "                                           fasta/<gene>/nj.nwk; the others are external programs and are refused [default: iqtree]\n"
         "  -p, --tree-options <TREE_OPTIONS>        Options for tree builder; nj: \"--model kimura|p\" [default: kimura], \"--bootstrap B\" replicates label\n"
         "                                           every internal branch with its support in percent [default: 0], \"--seed S\" of their draws\n"
         "                                           [default: 1], \"--support fbp|tbe\" the share of replicates with the same branch or the\n"
         "                                           transfer bootstrap expectation [default: fbp], the same for every gene\n"
         "  -f, --realign                            Refused: re-aligning single genes is not built in\n"
         "  -c, --threads <THREADS>                  Number of threads to use; 0 to use all [default: 0]\n"
         "  -v, --verbosity <VERBOSITY>              Verbosity (0: quiet, 1: +errors, 2: +warnings, 3: +info, 4: +debug) [default: 3]\n"
         "  -h, --help                               Print help\n", to);
}

[[noreturn]] void clap_error_gene_tree(const std::string &what) {
    fprintf(stderr, "error: %s\n\nUsage: unicore gene-tree [OPTIONS] --tree-builder nj <INPUT>\n\nFor more information, try '--help'.\n", what.c_str());
    exit(CLAP_USAGE);
}

// Commands::GeneTree (arg_parser.rs:334-367) + modules::genetree::run (genetree.rs:9-147) with the built-in builder: one tree per gene of a tree output
// directory, fasta/<gene>/<gene>.fa.filtered -> fasta/<gene>/nj.nwk.  The reference walks read_dir; here the genes are taken in ascending byte order.
int gene_tree_main(int argc, char **argv) {
    std::vector<std::string> pos;
    std::string builder = "iqtree", tree_options, names;
    bool realign = false;
    int verbosity = 3, threads = 0;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto value = [&]() -> std::string {
            if (i + 1 >= argc) clap_error_gene_tree("a value is required for '" + a + "' but none was supplied");
            return argv[++i];
        };
        if (a == "-t" || a == "-T" || a == "--tree-builder") builder = value();
        else if (a.rfind("--tree-builder=", 0) == 0) builder = a.substr(15);
        else if (a == "-n" || a == "--names") names = value();
        else if (a.rfind("--names=", 0) == 0) names = a.substr(8);
        else if (a == "-p" || a == "--tree-options") tree_options = value();
        else if (a.rfind("--tree-options=", 0) == 0) tree_options = a.substr(15);
        else if (a == "-f" || a == "--realign") realign = true;
        else if (a == "-a" || a == "--aligner" || a == "-o" || a == "--aligner-options" || a == "-d" || a == "--threshold") (void)value();      // read by --realign only
        else if (a == "-c" || a == "--threads") threads = atoi(value().c_str());      // read by the bootstrap of nj alone
        else if (a == "-v" || a == "--verbosity") verbosity = atoi(value().c_str());
        else if (a == "-h" || a == "--help") { usage_gene_tree(stdout); return 0; }
        else if (a.size() > 1 && a[0] == '-') clap_error_gene_tree("unexpected argument '" + a + "' found");
        else pos.push_back(a);
    }
    if (pos.empty()) clap_error_gene_tree("the following required arguments were not provided");
    if (pos.size() > 1) clap_error_gene_tree("unexpected argument '" + pos[1] + "' found");
    if (verbosity < 0 || verbosity > 4) clap_error_gene_tree("invalid value for '--verbosity <VERBOSITY>'");
    g_verbosity = verbosity;
    const std::string input = pos[0], fasta = input + "/fasta";
    struct stat sb;
    if (stat(input.c_str(), &sb) != 0) error(ERR_GENERAL, "Input directory does not exist");                                             // genetree.rs:22-24
    if (stat(fasta.c_str(), &sb) != 0) error(ERR_GENERAL, "Input directory does not contain core structure fasta directories");          // genetree.rs:27-29
    if (builder == "iqtree" || builder == "fasttree" || builder == "raxml-ng") refuse_external_builder(builder);
    if (builder != "nj") error(ERR_GENERAL, "Unrecognized tree builder");                                                                // genetree.rs:47
    const NjOptions nj_opts = nj_options_of(tree_options);      // every gene draws under the same seed
    if (realign) error(ERR_GENERAL, "--realign would align every gene again, which gene-tree does not do in this build; run `unicore tree` for a new alignment");
    std::vector<std::string> wanted;
    if (!names.empty()) {                                                                                                                // genetree.rs:52-61
        std::ifstream f(names);
        if (!f) error(ERR_GENERAL, "Names file does not exist");
        for (std::string line; std::getline(f, line);) { if (!line.empty() && line.back() == '\r') line.pop_back(); wanted.push_back(line); }
    }
    std::vector<std::string> genes;
    DIR *d = opendir(fasta.c_str());
    if (!d) error(ERR_GENERAL, "Input directory does not contain core structure fasta directories");
    while (const dirent *e = readdir(d)) {
        const std::string g = e->d_name;
        if (g != "." && g != "..") genes.push_back(g);
    }
    closedir(d);
    std::sort(genes.begin(), genes.end());
    if (!wanted.empty()) {                                                                                                               // genetree.rs:72-83
        std::vector<std::string> kept;
        for (const std::string &g : genes) {
            const std::string stem = g.substr(0, g.rfind('.') == std::string::npos || g.rfind('.') == 0 ? g.size() : g.rfind('.'));      // Path::file_stem
            if (std::find(wanted.begin(), wanted.end(), stem) != wanted.end()) kept.push_back(g);
        }
        if (kept.empty()) error(ERR_GENERAL, "No gene names matched");
        genes = kept;
    }
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.threads = 1;
    o.verbosity = verbosity;
    o.device = -1;
    print_message("\rInferring gene specific phylogenetic trees 0/" + std::to_string(genes.size()) + "...", 3);                          // genetree.rs:112
    for (size_t k = 0; k < genes.size(); k++) {
        const std::string dir = fasta + "/" + genes[k], msa = dir + "/" + genes[k] + ".fa.filtered";
        size_t rows = 0;
        {
            std::ifstream f(msa, std::ios::binary);
            const bool opened = (bool)f;
            if (opened) for (std::string line; std::getline(f, line);) rows += !line.empty() && line[0] == '>';
            else if (g_verbosity >= 2) fprintf(stderr, "\nWarning: gene %s has no filtered alignment %s; it gets no tree\n", genes[k].c_str(), msa.c_str());
            if (opened && rows < 2 && g_verbosity >= 2) fprintf(stderr, "\nWarning: gene %s has %zu row(s); a tree needs two; it gets no tree\n", genes[k].c_str(), rows);
        }
        if (rows >= 2) {
            const int rc = nj_infer(msa, dir + "/nj.nwk", nj_opts, o, threads);
            if (rc != 0) error(ERR_GENERAL, "gene-tree failed on " + genes[k] + " with code " + std::to_string(rc) + "\n" + uc_last_error());
        }
        print_message("\rInferring gene specific phylogenetic trees " + std::to_string(k + 1) + "/" + std::to_string(genes.size()) + "...", 3);   // genetree.rs:142
    }
    println_message("Done", 3);                                                                                                           // genetree.rs:144
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) { usage(stderr); return CLAP_USAGE; }
    if (!strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) { usage(stdout); return 0; }
    if (!strcmp(argv[1], "version") || !strcmp(argv[1], "--version")) { puts(uc_version()); return 0; }
    if (!strcmp(argv[1], "profile")) {
        const int rc = profile_main(argc, argv);
        fflush(stdout);
        fflush(stderr);
        _exit(rc);
    }
    if (!strcmp(argv[1], "tree") && argc > 2) {      // bare `unicore tree` keeps its earlier answer below (ERR_MODULE_NOT_IMPLEMENTED)
        const int rc = tree_main(argc, argv);
        fflush(stdout);
        fflush(stderr);
        _exit(rc);
    }
    if (!strcmp(argv[1], "gene-tree") && argc > 2) {      // the bare module name keeps its earlier answer below
        const int rc = gene_tree_main(argc, argv);
        fflush(stdout);
        fflush(stderr);
        _exit(rc);
    }
    const bool is_search = !strcmp(argv[1], "search");
    if (strcmp(argv[1], "cluster") != 0 && !is_search) error(0x30 /* ERR_MODULE_NOT_IMPLEMENTED */, argv[1]);
    if (argc == 2) { if (is_search) usage_search(stderr); else usage(stderr); return CLAP_USAGE; }   // arg_required_else_help
    std::vector<std::string> pos;
    bool keep = false;
    std::string copts = "-c 0.8";   // arg_parser.rs:238-239 (cluster), :262-263 (search)
    int threads = 0, verbosity = 3;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i];
        auto value = [&]() -> std::string {
            if (i + 1 >= argc) clap_error(is_search, "a value is required for '" + a + "' but none was supplied");
            return argv[++i];
        };
        if (a == "-k" || a == (is_search ? "--keep-aln-db" : "--keep-cluster-db")) keep = true;
        else if (!is_search && (a == "-c" || a == "--cluster-options")) copts = value();
        else if (!is_search && a.rfind("--cluster-options=", 0) == 0) copts = a.substr(18);
        else if (is_search && (a == "-s" || a == "--search-options")) copts = value();
        else if (is_search && a.rfind("--search-options=", 0) == 0) copts = a.substr(17);
        else if (a == "--threads") threads = atoi(value().c_str());
        else if (a == "-v" || a == "--verbosity") verbosity = atoi(value().c_str());
        else if (a == "-h" || a == "--help") { if (is_search) usage_search(stdout); else usage(stdout); return 0; }
        else if (a.size() > 1 && a[0] == '-') clap_error(is_search, "unexpected argument '" + a + "' found");
        else pos.push_back(a);
    }
    const size_t want = is_search ? 4 : 3;
    if (pos.size() < want) clap_error(is_search, "the following required arguments were not provided");
    if (pos.size() > want) clap_error(is_search, "unexpected argument '" + pos[want] + "' found");
    if (verbosity < 0 || verbosity > 4) clap_error(is_search, "invalid value for '--verbosity <VERBOSITY>'");
    g_verbosity = verbosity;
    // set_threads (variables.rs:155-166): 0 -> all CPUs, clamp to the CPU count
    int cpus = (int)std::thread::hardware_concurrency();
    if (cpus < 1) cpus = 1;
    if (threads > cpus) {
        if (g_verbosity >= 2) fprintf(stderr, "Warning: the given number of threads is greater than the number of system CPUs; adjusting to %d\n", cpus);
        threads = cpus;
    }
    if (threads <= 0) threads = cpus;
    const int rc = is_search ? search_run(pos[0], pos[1], pos[2], pos[3], keep, copts, threads) : cluster_run(pos[0], pos[1], pos[2], keep, copts, threads);
    // outputs and the checkpoint are on disk: skip the teardown of the HIP runtime and its parked work buffers (~0.1 s per call)
    fflush(stdout);
    fflush(stderr);
    _exit(rc);
}
