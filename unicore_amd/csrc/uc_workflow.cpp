// uc_workflow.cpp — the driver of a `unicore cluster` run (uc_workflow.h): one ClusterRun per call, one Rank per GPU.  Rank 0 owns the workflow
// (which sequences a round sees, its k-score, the merge of its clustering); the other ranks follow its rounds from barrier to barrier.  Every
// rank passes the same barriers in the same order on every path: a rank that throws fails the group instead (run_ranks).
#include "uc_workflow.h"

#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <thread>

#include "uc_engine.h"
#include "uc_files.h"
#include "uc_multi.h"

namespace uc {

namespace {

std::mutex g_hook_mu;
uc_round_hook g_round_hook = nullptr;
void *g_round_hook_user = nullptr;

void call_round_hook(Engine &E, int round, const std::vector<uint32_t> &ids) {
    uc_round_hook h; void *u;
    { std::lock_guard<std::mutex> lk(g_hook_mu); h = g_round_hook; u = g_round_hook_user; }
    if (!h) return;
    uc_engine view;                       // a non-owning view of the round's engine for the duration of the call
    view.e.reset(&E);
    struct Release { uc_engine &v; ~Release() { (void)v.e.release(); } } rel{view};
    h(u, round, E.hdb.n, ids.data(), E.p.kmer_thr, &view);
}

// what one rank's thread owns
struct Rank {
    Engine E;
    Comm &C;
    const int r;
    Timer tph;      // since the last UC_TIMING stamp of this rank
    Rank(const Params &p, int device, Comm &c, int rank) : E(p, device), C(c), r(rank) {}
};

struct ClusterRun {
    // ---- state shared by the rank threads (host memory; rank 0 writes it between two barriers, the others read it after the second)
    Params p;
    std::vector<int> devices;
    int W = 1, gT = 1;
    bool virtual_gpus = false;
    HostDb full, round_db;                 // the database; the sub-database of the round (rounds > 0, several ranks)
    std::vector<uint32_t> assign, cur, posmap;
    std::vector<uint32_t> pre_pairs;       // candidate pairs of the pre-step
    int round_kmer_thr = 0;
    std::unique_ptr<LocalGroup> grp;
    std::vector<std::unique_ptr<Comm>> comms;
    std::vector<uc_stats> rank_stats;
    uint64_t n_clusters = 0;
    uint32_t nccl_ranks = 0;
    // ---- fixed once open() has returned
    const bool timing = getenv("UC_TIMING") != nullptr;
    uint32_t n = 0;
    int pre = 0, rounds = 0;               // E8a: one linear-time pre-clustering round in front of the cascade rounds
    double t_load = 0;
    std::future<void> preload;             // last member: its destructor joins the helper thread before anything above goes away

    void mark(const char *what) const {
        if (timing) fprintf(stderr, "unicore-cluster[timing]: t+%7.1f ms  %s\n", 1e3 * g_library_loaded.seconds(), what);
    }
    void phase(Rank &k, const char *what, int rr) const {
        if (timing && k.r == 0) fprintf(stderr, "unicore-cluster[timing]: t+%7.1f ms  round %d %-14s %.1f ms\n", 1e3 * g_library_loaded.seconds(), rr, what, 1e3 * k.tph.seconds());
        k.tph = Timer();
    }
    std::vector<Comm *> comm_ptrs() const {
        std::vector<Comm *> cs;
        for (auto &c : comms) cs.push_back(c.get());
        return cs;
    }

    // A single rank BORROWS the database instead of copying it: `full` moves into the engine for round 0 and comes back when the engine lays
    // the next round's sub-database out on the device (rr == 1), or at the end of a one-round run.  No host copy of the database, ever, on one rank.
    void lend_db(Engine &E) { E.hdb = std::move(full); }
    void reclaim_db(Engine &E) { full = std::move(E.hdb); }

    // The HIP runtime and the device context take 0.15-0.3 s to come up in a fresh process (tools/cold_stamps.sh): they are initialised on
    // a helper thread WHILE this thread reads and encodes the database (a one-shot `foldseek cluster` process pays for both every time).
    // Returns the number of visible devices.
    int read_db_beside_warmup(const char *db, int want_dev) {
        std::future<int> warm = std::async(std::launch::async, [want_dev]() -> int {
            int nd = 0;
            if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return 0;
            if (hipSetDevice(want_dev < nd ? want_dev : 0) == hipSuccess) (void)hipFree(nullptr);      // forces the primary context into existence
            return nd;
        });
        Timer tl;
        logf(3, "unicore-cluster: reading %s\n", db);
        read_seq_db(db, full, false);
        t_load = tl.seconds();
        mark("database read + encoded");
        const int ndev = warm.get();
        if (ndev <= 0) fail(UC_ERR_DEVICE, "no HIP device available; this engine has no CPU fallback");
        mark("HIP runtime + device context ready (initialised beside the database read)");
        return ndev;
    }

    // what the rank threads share, before the first of them starts
    void init_shared_state() {
        assign.resize(n); cur.resize(n); posmap.resize(n);
        for (uint32_t i = 0; i < n; i++) { assign[i] = i; cur[i] = i; }
        round_kmer_thr = p.kmer_thr;
        grp.reset(new LocalGroup(W));
        if (virtual_gpus && getenv("UC_VIRTUAL_SERIAL")) grp->serialize = true;   // emulation: one rank's compute phase at a time on the shared GPU
        for (int r = 0; r < W; r++) {
            comms.emplace_back(new Comm);
            comms.back()->rank = r; comms.back()->world = W; comms.back()->grp = W > 1 ? grp.get() : nullptr;
        }
        rank_stats.resize((size_t)W);
    }

    // false: the database is empty and the (empty) cluster DB is written
    bool open(const char *db, const char *out, const char *tmp, const uc_opts *o, uc_stats *stats_out) {
        mark("uc_cluster entered");
        p = params_from(o);
        mark("options + matrices");
        if (tmp && *tmp) make_dirs(tmp);   // callee owns <tmp>; nothing is spilled there yet
        if (p.mat3di_synthetic)
            logf(1, "Warning: clustering with the SYNTHETIC 3Di matrix %s (UC_ALLOW_SYNTHETIC=1): results are not Foldseek's\n", p.mat3di_path.c_str());
        const int ndev = read_db_beside_warmup(db, o && o->device >= 0 ? o->device : 0);
        DevicePlan plan = plan_visible_devices(p.num_gpus, o ? o->device : -1, ndev);
        W = plan.world; devices = std::move(plan.devices); virtual_gpus = plan.virtual_gpus;
        int gQ = 1;
        grid_shape(W, p.target_shards, &gQ, &gT);
        n = full.n;
        if (n == 0) {   // an empty, well-formed database: an empty cluster DB, whatever the workflow
            write_cluster_db(out, full.keys, nullptr, 0);
            logf(3, "unicore-cluster: empty database -> %s\n", out);
            if (stats_out) { *stats_out = uc_stats(); stats_out->n_gpus = (uint32_t)W; stats_out->target_shards = (uint32_t)gT; stats_out->stage_seconds[UC_ST_LOAD] = t_load; }
            return false;
        }
        pre = p.linclust ? 1 : 0;
        rounds = p.cluster_steps + pre;
        // the kernels' code objects are uploaded on a helper thread beside engine construction, database upload and prefilter (uc_sw.hip:preload_modules)
        if (W == 1)
            preload = std::async(std::launch::async, [d0 = devices[0], lc = pre != 0, st = timing]() {
                preload_modules(d0, lc);
                if (st) fprintf(stderr, "unicore-cluster[timing]: t+%7.1f ms  (helper thread) code objects of the prefilter / alignment / SW modules loaded\n", 1e3 * g_library_loaded.seconds());
            });
        logf(3, "unicore-cluster: %u sequences, %llu residues, %d GPU(s)%s [%d query group(s) x %d target shard(s)], %s%d clustering step(s)\n", n,
             (unsigned long long)full.residues(), W, virtual_gpus ? " (virtual: several ranks per device)" : "", gQ, gT,
             pre ? "linear-time pre-step + " : "", p.cluster_steps);
        init_shared_state();
        return true;
    }

    // every engine exists (a constructor that threw has failed the group: this barrier then throws on the others) BEFORE any rank enters RCCL;
    // rank 0 then creates all communicators in one call — a collective init per rank would leave the survivors of a failed peer blocked
    // inside ncclCommInitRank for good
    void connect(Rank &k) {
        grp->barrier();
        if (k.r == 0 && !virtual_gpus) {
            comm_init_all(comm_ptrs(), devices);
            int cnt = 0, rk = 0, dv = 0;
            comm_info(k.C, &cnt, &rk, &dv);
            nccl_ranks = (uint32_t)cnt;
            logf(3, "unicore-cluster: RCCL communicator over %d ranks (ncclCommCount)\n", cnt);
        }
        grp->barrier();
    }

    // rank 0 decides what the round sees; then every rank loads it.  rr counts the pre-step, rd = rr - pre is the cascade round (-1 = the pre-step)
    void begin_round(Rank &k, int rr) {
        Engine &E = k.E;
        const int rd = rr - pre;
        if (W == 1 && rr == 1) reclaim_db(E);
        const bool dev_sub = W == 1 && rr > 0;      // a single rank lays the representatives' sub-database out on the device
        if (k.r == 0) {
            if (rr > 0 && !dev_sub) round_db = sub_db(full, cur);
            round_kmer_thr = p.kmer_thr;
            if (rd >= 0 && p.cluster_steps > 1 && !p.kmer_thr_explicit)   // sensitivity rises linearly from 1 to the target (spec UC-1 E8)
                round_kmer_thr = kmer_thr_for(p, 1.0 + (p.sensitivity - 1.0) * rd / (p.cluster_steps - 1));
        }
        k.C.barrier(E);
        phase(k, "sub_db", rr);
        if (W == 1 && rr == 0) lend_db(E);
        else if (W > 1) E.hdb = rr == 0 ? full : round_db;
        phase(k, "hdb copy", rr);
        E.p.kmer_thr = round_kmer_thr;
        if (dev_sub) E.upload_sub_db(cur, full.off);
        else E.upload_db(/*keep_raw=*/W == 1 && rounds > 1);
        phase(k, "upload", rr);
    }

    // E8a: candidate pairs (centre, member) from shared minimum-hash k-mers become the hit lists, the centre is the query
    void hits_of_pre_step(Rank &k, int rr) {
        Engine &E = k.E;
        const uint32_t m = E.hdb.n;
        if (W == 1) {   // one rank: without leaving the device
            const uint64_t np = E.linclust_hits();
            phase(k, "linclust_pairs", rr);
            E.stats.n_prefilter_hits += np;
            logf(3, "unicore-cluster: pre-step: %u sequences, %llu candidate pairs (%d k-mers per sequence)\n", m, (unsigned long long)np, p.kmer_per_seq);
            return;
        }
        if (k.r == 0) pre_pairs = E.linclust_pairs();
        phase(k, "linclust_pairs", rr);
        k.C.barrier(E);
        // a rank aligns the pairs of the centres it owns (centre mod world): whole queries stay together
        std::vector<uint32_t> cnt(m, 0);
        std::vector<uc_hit> hl;
        hl.reserve(pre_pairs.size() / 2 / (size_t)W + 16);
        for (size_t i = 0; i < pre_pairs.size() / 2; i++) {
            const uint32_t c = pre_pairs[2 * i];
            if ((int)(c % (uint32_t)W) != k.r) continue;
            cnt[c]++;
            uc_hit h; h.target = pre_pairs[2 * i + 1]; h.score = 0; h.diag = 0;
            hl.push_back(h);
        }
        E.set_hits(cnt.data(), hl.data(), /*check_max_seqs=*/false);
        E.stats.n_prefilter_hits += hl.size();
        if (k.r == 0)
            logf(3, "unicore-cluster: pre-step: %u sequences, %zu candidate pairs (%d k-mers per sequence)\n", m, pre_pairs.size() / 2, p.kmer_per_seq);
    }

    void hits_of_round(Rank &k, int rd) {
        Engine &E = k.E;
        prefilter_turn(E, k.C, p.target_shards);
        if (inject_failure(k.r, 1)) fail(UC_ERR_DEVICE, "injected failure of rank %d (UC_FAIL_RANK)", k.r);
        if (W > 1) exchange_hits(E, k.C);
        if (k.r == 0)
            logf(3, "unicore-cluster: step %d: %u sequences, prefilter kept %llu pairs%s (k-score %d, max-seqs %d)\n", rd + 1, E.hdb.n,
                 (unsigned long long)E.n_hits, W > 1 ? " on rank 0" : "", E.p.kmer_thr, p.max_seqs);
    }

    // accepted edges of every rank -> the round's clustering of the representatives -> merged into the run's (rank 0)
    void cover_and_merge(Rank &k, int rd) {
        Engine &E = k.E;
        const uint32_t m = E.hdb.n;
        std::vector<uint32_t> sa(k.r == 0 ? m : 0);
        const uint64_t n_acc = round_graph(E, k.C, m, sa.data());
        if (k.r != 0) return;
        Timer tm;      // the merge counts as set-cover time too
        std::vector<uint32_t> next = merge_round(assign, cur, sa, posmap);
        E.stats.stage_seconds[UC_ST_SETCOVER] += tm.seconds();
        if (W > 1) E.stats.phase_seconds[7] += tm.seconds();
        logf(3, "unicore-cluster: step %d: %llu accepted pairs, %zu representatives\n", rd + 1, (unsigned long long)n_acc, next.size());
        cur.swap(next);
        E.stats.n_edges = n_acc;
    }

    // rule UC-1/R on rank 0's engine alone (the others wait at the final barrier: the rejected sets are small).  The full database becomes the
    // engine's again: one rank lays it out from the raw copy the rounds kept on the device (or still holds it after a plain step)
    void reassign_final(Rank &k) {
        Engine &E = k.E;
        phase(k, "(between)", rounds);
        Timer tr;
        E.p.kmer_thr = p.kmer_thr;                    // the final sensitivity, not a cascade round's
        if (W == 1 && rounds > 1) {
            std::vector<uint32_t> all(n);
            for (uint32_t i = 0; i < n; i++) all[i] = i;
            E.upload_sub_db(all, full.off);
        } else if (W > 1) {
            E.hdb = full;
            E.upload_db(/*keep_raw=*/true);
        }
        std::vector<uint32_t> out(n);
        uint64_t rc[4] = {0, 0, 0, 0};
        const uint64_t before = cur.size();
        E.reassign(assign.data(), out.data(), nullptr, rc);
        assign.swap(out);
        cur.clear();
        for (uint32_t x = 0; x < n; x++) if (assign[x] == x) cur.push_back(x);
        logf(3, "unicore-cluster: reassign: %llu members verified, %llu rejected, %llu re-search pairs accepted, %llu -> %zu clusters (%.1f ms)\n",
             (unsigned long long)rc[0], (unsigned long long)rc[1], (unsigned long long)rc[2], (unsigned long long)before, cur.size(), 1e3 * tr.seconds());
        phase(k, "reassign", rounds);
    }

    void rank_main(int r) {
        Rank k(p, devices[(size_t)r], *comms[(size_t)r], r);
        if (r == 0) mark("engine constructed (streams, events, matrices on the device)");
        if (inject_failure(r, 0)) fail(UC_ERR_DEVICE, "injected failure of rank %d (UC_FAIL_RANK)", r);
        if (W > 1) connect(k);
        k.tph = Timer();
        for (int rr = 0; rr < rounds; rr++) {
            phase(k, "(between)", rr);
            begin_round(k, rr);
            if (rr < pre) hits_of_pre_step(k, rr);
            else hits_of_round(k, rr - pre);
            phase(k, "hits", rr);
            align_turn(k.E, k.C, k.E.hdb.n);
            phase(k, "align", rr);
            if (r == 0) call_round_hook(k.E, rr - pre, cur);
            cover_and_merge(k, rr - pre);
            phase(k, "cover+merge", rr);
        }
        if (r == 0 && p.reassign) reassign_final(k);
        k.C.barrier(k.E);
        if (W == 1 && rounds == 1) reclaim_db(k.E);
        if (r == 0) n_clusters = cur.size();
        rank_stats[(size_t)r] = k.E.stats;
    }

    void run_ranks() {
        if (W == 1) { rank_main(0); return; }
        std::vector<std::string> err((size_t)W);
        std::vector<int> code((size_t)W, 0);
        std::vector<std::thread> th;
        // a rank on its way out fails the group (peers leave their next barrier with an error) and aborts every RCCL
        // communicator (peers blocked INSIDE a collective return from it)
        auto bail = [this] { grp->fail_all(); abort_all(comm_ptrs()); };
        for (int r = 0; r < W; r++)
            th.emplace_back([&, r] {
                try { rank_main(r); }
                catch (const Error &e) { code[(size_t)r] = e.code; err[(size_t)r] = e.what(); bail(); }
                catch (const std::exception &e) { code[(size_t)r] = UC_ERR_GENERIC; err[(size_t)r] = e.what(); bail(); }
            });
        for (auto &t : th) t.join();
        // report the rank that failed first-hand, not the ones that were released from a barrier because of it
        int bad = -1;
        for (int r = 0; r < W; r++)
            if (code[(size_t)r] && (bad < 0 || err[(size_t)bad].find("another GPU rank") != std::string::npos)) bad = r;
        if (bad >= 0) fail(code[(size_t)bad], "GPU rank %d: %s", bad, err[(size_t)bad].c_str());
    }

    void finish(const char *out, uc_stats *stats_out) {
        uc_stats st = rank_stats[0];
        for (int r = 1; r < W; r++) merge_stats(st, rank_stats[(size_t)r]);
        st.stage_seconds[UC_ST_LOAD] += t_load;
        st.n_clusters = n_clusters;
        st.n_seqs = n;
        st.n_residues = full.residues();
        st.n_gpus = (uint32_t)W;
        st.target_shards = (uint32_t)gT;
        st.nccl_ranks = nccl_ranks;
        Timer to;
        write_cluster_db(out, full.keys, assign.data(), n);
        st.stage_seconds[UC_ST_OUTPUT] += to.seconds();
        mark("cluster DB written");
        logf(3, "unicore-cluster: %llu clusters -> %s\n", (unsigned long long)n_clusters, out);
        if (stats_out) *stats_out = st;
    }
};

}  // namespace

void set_round_hook(uc_round_hook hook, void *user) {
    std::lock_guard<std::mutex> lk(g_hook_mu);
    g_round_hook = hook; g_round_hook_user = user;
}

DevicePlan plan_visible_devices(int want, int device, int ndev) {
    int cur = 0;
    if ((want == 1 || (want == 0 && ndev == 1)) && device < 0) UC_HIP(hipGetDevice(&cur));      // asked only where the plan needs it: one rank, no device named
    const char *v = getenv("UC_VIRTUAL_GPUS");
    return plan_devices(want, device, cur, ndev, v && strcmp(v, "1") == 0);
}

void cluster_workflow(const char *db, const char *out, const char *tmp, const uc_opts *o, uc_stats *stats_out) {
    ClusterRun run;
    if (!run.open(db, out, tmp, o, stats_out)) return;
    run.run_ranks();
    run.finish(out, stats_out);
}

}  // namespace uc
