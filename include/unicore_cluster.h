/* unicore_cluster.h — C ABI of the MI355X-native `unicore cluster` engine (libunicore_cluster.so).
 *
 * This is the drop-in boundary for the ONE hot path of steineggerlab/unicore: the three external
 * `foldseek` invocations of /root/reference/src/modules/cluster.rs:45-76.  The reference has no
 * in-process FFI for this path (its extension point is the binary registry path.cfg:2 +
 * src/util/command.rs:4-24), so the entry points below are exactly what a Rust `unicore` would bind
 * with `extern "C"` to replace those three spawns (INTEGRATION.md shows the binding), plus a staged
 * engine API used by the multi-GPU driver, bench.py and the parity tests.
 *
 * Conventions: plain pointers and sizes, caller-owned memory unless stated, UTF-8 paths, no
 * exceptions cross the boundary.  Every int-returning function returns 0 on success or an error class
 * (exit status is the reference's only error channel: src/util/command.rs:10-14):
 *     1 generic, 2 bad arguments / unknown flag, 3 I/O, 4 device (HIP) failure or no GPU.
 * uc_last_error() gives the message (thread-local).  There is NO CPU fallback: without a working HIP
 * device every compute entry point fails with class 4.
 */
#ifndef UNICORE_CLUSTER_H
#define UNICORE_CLUSTER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define UC_OK 0
#define UC_ERR_GENERIC 1
#define UC_ERR_ARGS 2
#define UC_ERR_IO 3
#define UC_ERR_DEVICE 4

/* Options.  `cluster_options` is the raw whitespace-split Foldseek-style flag string that
 * src/modules/cluster.rs:35,49 forwards verbatim (default "-c 0.8", src/util/arg_parser.rs:238-239).
 * Unknown flags are rejected (UC_ERR_ARGS), never ignored. */
typedef struct uc_opts {
    uint32_t struct_size;        /* = sizeof(uc_opts) */
    int32_t threads;             /* host threads, >=1 (cluster.rs:46 "--threads") */
    int32_t verbosity;           /* 0..3, Foldseek scale after the 4->3,3->2 mapping of cluster.rs:18 */
    int32_t device;              /* HIP device ordinal of a single-GPU run / of an engine, -1 = current */
    int32_t num_gpus;            /* uc_cluster, uc_createdb: GPUs the run is spread over: 0 = all visible, 1 = `device`,
                                    N = devices 0..N-1; "--gpus N" inside cluster_options overrides it (uc_cluster) */
    const char *cluster_options; /* may be NULL == "" */
    const char *data_dir;        /* directory holding mat3di.out / blosum62.out; NULL = <lib dir>/data.  Without a real
                                    mat3di.out the call fails unless UC_ALLOW_SYNTHETIC=1 opts into the seeded stand-in */
} uc_opts;

/* ABI revision of this header: bumped whenever a struct below grows or an entry point changes meaning.  uc_stats is written in full by
 * uc_cluster / uc_search / uc_engine_stats and carries no size field of its own, so a caller built against an older header must check
 * uc_abi_version() == UC_ABI_VERSION (or uc_stats_size() == sizeof(uc_stats)) before passing one in. */
#define UC_ABI_VERSION 9
uint32_t uc_abi_version(void);
size_t uc_stats_size(void);

#define UC_NSTAGE 8
enum { UC_ST_LOAD = 0, UC_ST_INDEX = 1, UC_ST_KMER = 2, UC_ST_UNGAPPED = 3, UC_ST_SELECT = 4,
       UC_ST_GAPPED = 5, UC_ST_SETCOVER = 6, UC_ST_OUTPUT = 7 };

#define UC_NPHASE 8
typedef struct uc_stats {
    uint64_t n_seqs, n_residues;
    uint64_t n_index_entries, n_sim_kmers, n_kmer_hits, n_candidates, n_prefilter_hits;
    uint64_t n_gapped_alignments;        /* (query,target) pairs handed to stage E5: the metric's unit */
    uint64_t n_start_alignments;         /* pairs that also ran the start-position pass */
    uint64_t n_pk_reruns;                /* alignment-passes of the packed 16-bit kernel re-run in int32 */
    uint64_t n_edges, n_clusters;
    uint64_t cells_fwd, cells_rev, cells_start;          /* DP cell updates per pass */
    uint64_t algorithmic_bytes[UC_NSTAGE];               /* SURVEY.md 8(d) per-stage algorithmic bytes */
    double stage_seconds[UC_NSTAGE];                     /* host wall per stage */
    /* dominant kernel (gapped SW, all passes): HIP-event time on the engine stream */
    double sw_kernel_ms;
    uint64_t sw_kernel_launches;
    uint64_t sw_algorithmic_bytes;                       /* sum over launches of 2*(Lq+Lt)+32 per alignment-pass */
    double prefilter_kernel_ms;                          /* all prefilter kernels (HIP events) */
    uint64_t n_filtered_hits;                            /* k-mer hits that survive the double-hit filter and get sorted */
    uint64_t n_sw_runs;                                  /* DP problems actually executed over all passes (mutual hits share one, re-runs add) */
    uint64_t cells_run;                                  /* DP cell updates actually executed (cells_* above are the algorithmic counts) */
    /* multi-GPU exchange: wall seconds of the two hit-list exchanges (shard lists to the query's home rank, surviving
     * pairs to their owner rank) + device merges + edge gather on this rank, and the bytes this rank received from its peers */
    double exchange_seconds;
    uint64_t exchange_bytes;
    uint32_t n_gpus, target_shards;                      /* the Q x T grid the run used: Q = n_gpus / target_shards */
    /* N > 1 only: wall seconds of this rank per phase of the sharded pass (uc_cluster reports the slowest rank per phase):
     * [0] prefilter of the rank's grid cell, [1] exchange 1 (shard lists to the query's home rank), [2] merge + top-M at home,
     * [3] partition by owner + exchange 2 (surviving pairs to their owner rank), [4] install of the owned lists, [5] gapped stage,
     * [6] edge gather to rank 0, [7] rank 0's serial tail (graph + greedy cover) */
    double phase_seconds[UC_NPHASE];
    uint32_t nccl_ranks, reserved0;                      /* ncclCommCount of the run's communicator (0 = no RCCL: one GPU or virtual ranks) */
    /* phase [3] taken apart (ABI 5): [0] stable partition of the merged pairs by owner rank (device sort), [1] exchange of the per-peer counts
     * (a small all-gather: it ends when the SLOWEST rank has finished its partition), [2] waiting at the rendezvous of the data exchange
     * (in-process ranks: the barriers around the device copies; RCCL ranks: 0 - the wait is inside the stream synchronisation of [3]),
     * [3] the data movement itself (grouped ncclSend / ncclRecv + stream synchronisation, or the device copies of in-process ranks) */
    double exchange2_seconds[4];
    /* (ABI 5) DP cells of the traceback boxes [qStart..qEnd] x [tStart..tEnd] of every pair whose statistics were asked for (--min-seq-id, search):
     * the fourth pass of the spec; cells_fwd + cells_rev + cells_start + cells_tb is what cells_run has to be read against */
    uint64_t cells_tb;
} uc_stats;

/* ---- the three calls of cluster.rs ------------------------------------------------------------ */
/* == `foldseek cluster --threads T -v V <db> <out>_cluster <tmp> <opts...>`  (cluster.rs:45-56) */
int uc_cluster(const char *db, const char *out_cluster_db, const char *tmp, const uc_opts *o, uc_stats *stats_out);
/* == `foldseek createtsv --threads T -v V <db> <db> <out>_cluster <out>.tsv`   (cluster.rs:59-64) */
int uc_createtsv(const char *db, const char *cluster_db, const char *out_tsv, const uc_opts *o);
/* == `foldseek rmdb <out>_cluster -v V`                                         (cluster.rs:67-76) */
int uc_rmdb(const char *db_prefix);

/* Workflow observer (optional).  A bare "-c 0.8" — what cluster.rs:35,49 forwards — runs the DEFAULT workflow: a linear-time pre-step and a
 * 3-step cascade, each round on the representatives of the one before.  A registered hook is called by uc_cluster once per round, after the
 * round's gapped stage and before its set cover, on the calling thread (single-GPU runs; with N GPUs: rank 0's thread, and `round_engine`
 * holds rank 0's share of the pairs only).  round = -1 for the pre-step, 0.. for the cascade rounds; the round works on n_round_seqs
 * sequences, round-local index i = database sequence seq_ids[i]; kmer_thr is the round's k-mer score threshold (the sensitivity rises from
 * 1 to the target over the rounds).  round_engine is valid only during the call: its hit lists and alignment records are the round's
 * (uc_engine_hits_get_range / uc_engine_alns_get / uc_engine_stats, round-local indices).  The at-size parity tests sample every round
 * against the CPU oracle through this; bench.py uses it to size the CPU baseline of the workflow round by round.  NULL unregisters. */
typedef struct uc_engine uc_engine;
typedef void (*uc_round_hook)(void *user, int32_t round, uint32_t n_round_seqs, const uint32_t *seq_ids, int32_t kmer_thr, uc_engine *round_engine);
void uc_set_round_hook(uc_round_hook hook, void *user);

/* ---- the calls of src/modules/search.rs, same kernels, query DB vs target DB --------------- */
/* == `foldseek search --threads T <queryDB> <targetDB> <out>_aln <tmp> <opts...>`  (search.rs:44-50; note that Unicore
 *    passes its TARGET argument first, i.e. as Foldseek's query DB).  Defaults as for cluster except -e 10 and
 *    --max-seqs 1000; traceback statistics for every accepted pair. */
int uc_search(const char *query_db, const char *target_db, const char *out_aln_db, const char *tmp, const uc_opts *o, uc_stats *stats_out);
/* == `foldseek convertalis --threads T <queryDB> <targetDB> <out>_aln <out>.m8`    (search.rs:52-57) */
int uc_convertalis(const char *query_db, const char *target_db, const char *aln_db, const char *out_m8, const uc_opts *o);

/* ---- createdb's GPU stage (BASELINE configs[4]): ProstT5 AA -> 3Di on the matrix cores ---------------
 * == `foldseek createdb <fasta> <db> --prostt5-model <dir> [--gpu 1]` (src/modules/createdb.rs:157-166).  `model` is the
 * GGUF file or the directory holding prostt5-f16.gguf (createdb.rs:148).  Writes <db>, <db>_h, <db>_ss (predicted 3Di) with
 * their .index / .dbtype and <db>.lookup: the files uc_cluster / uc_search read.  Several FASTA files: one path per entry. */
typedef struct uc_t5_stats {
    uint64_t n_seqs, n_tokens;       /* tokens = residues + 2 per sequence (<AA2fold> ... </s>) */
    double flops;                    /* algorithmic FLOPs of the linear layers + attention */
    double gpu_ms;                   /* HIP-event time of the encoder passes (several replicas: the SLOWEST replica's - they run side by side) */
    /* (ABI 6) uc_createdb on N GPUs: one encoder replica per GPU, sequences sharded over them, no collective (uc_opts.num_gpus as for uc_cluster) */
    uint32_t n_replicas, reserved0;
    double gpu_ms_sum;               /* sum over the replicas (== gpu_ms for one) */
    uint64_t tokens_min_replica, tokens_max_replica;   /* balance of the dynamic dealing */
} uc_t5_stats;
int uc_createdb(const char *const *fasta_paths, int n_fasta, const char *out_db, const char *model, const uc_opts *o, uc_t5_stats *stats_out);
/* the encoder alone (no disk round trip: the codes go straight into uc_engine_set_db): */
typedef struct uc_t5 uc_t5;
int uc_t5_load(const char *model, int32_t device, uc_t5 **out);
void uc_t5_free(uc_t5 *m);
/* n sequences as residue letters, off[n + 1] byte offsets into aa; codes (one 3Di state 0..19 per residue, same offsets);
 * logits (nullable): 20 floats per residue */
int uc_t5_encode(uc_t5 *m, uint32_t n, const uint64_t *off, const char *aa, uint8_t *codes, float *logits);
int uc_t5_get_stats(const uc_t5 *m, uc_t5_stats *out);

const char *uc_last_error(void);
const char *uc_version(void);
/* validates a Foldseek-style option string without running anything (0 or UC_ERR_ARGS) */
int uc_check_options(const char *cluster_options);
/* how the engine's flag table reads one flag: 1 = takes a value, 2 = switch with an optional 0/1, -1 = unknown.  The argv
 * shim uses it to split Foldseek-style command lines with flags anywhere. */
int uc_option_arity(const char *flag);
/* Work buffers (tens of GB of HBM at bench scale) are parked per device when an engine is destroyed, so that the next
 * uc_cluster / engine of the process does not pay hipMalloc again (UC_KEEP_SCRATCH=0 disables parking).  An in-process
 * host that is done with the engine for now calls this to give the memory back.  Loading the library also sets
 * GPU_MAX_HW_QUEUES=8 in the process environment if the variable is unset (the class kernels of a pass run on 8 streams). */
void uc_release_scratch(void);

/* ---- staged engine API (multi-GPU driver, bench, parity tests) -------------------------------- */

typedef struct uc_hit {          /* one prefilter result (stage E4 output) */
    uint32_t target;
    int32_t score;               /* ungapped diagonal score, 0..255 */
    int32_t diag;                /* query pos - target pos of the best diagonal */
} uc_hit;

typedef struct uc_aln {          /* one gapped alignment result (stage E5/E6 output) */
    int32_t score, score_rev, corrected;
    int32_t qstart, qend, tstart, tend;    /* valid iff pass_evalue */
    int32_t aln_len, idents;               /* valid iff a seq-id threshold is active */
    int32_t pass_evalue, accepted;
    int32_t gap_opens;                     /* with aln_len/idents: number of gaps on the traceback (search path) */
} uc_aln;

int uc_engine_create(const uc_opts *o, uc_engine **out);
void uc_engine_destroy(uc_engine *e);
/* load <db>, <db>_ss, <db>_h (+ .index) from disk and upload both tracks to HBM */
int uc_engine_load_db(uc_engine *e, const char *db_prefix);
/* or hand over encoded sequences directly: codes 0..20, off has n+1 entries (bytes), no padding */
int uc_engine_set_db(uc_engine *e, uint32_t n, const uint64_t *off, const uint8_t *s3, const uint8_t *sa);
uint32_t uc_engine_num_seqs(const uc_engine *e);

/* E1-E4: index targets [tbegin,tend), match ALL queries against it, keep per-query top max_seqs */
int uc_engine_prefilter(uc_engine *e, uint32_t tbegin, uint32_t tend);
/* the same with the queries restricted to [qbegin,qend): query DB vs target DB inside one loaded set (search path) */
int uc_engine_prefilter_range(uc_engine *e, uint32_t tbegin, uint32_t tend, uint32_t qbegin, uint32_t qend);
/* hit lists live in the engine: counts[n_seqs], hits flat, grouped by query in query order */
int uc_engine_hits_size(const uc_engine *e, uint64_t *n_hits);
int uc_engine_hits_get(const uc_engine *e, uint32_t *counts, uc_hit *hits);
/* the same for the queries [qbegin,qend) only: counts may be NULL; hits must hold the sum of their counts (at BASELINE
 * configs[2] scale the whole list is gigabytes, a sample of queries is not) */
int uc_engine_hits_get_range(const uc_engine *e, uint32_t qbegin, uint32_t qend, uint32_t *counts, uc_hit *hits);
/* replace the engine's hit lists (counts[n_seqs] + flat hits grouped by query).  A list names a target once (spec E4): UC_ERR_ARGS for a
 * list that repeats one - the gapped stage would take the second entry for the mirror (t, q) of the first.  A refused list changes nothing. */
int uc_engine_hits_set(uc_engine *e, const uint32_t *counts, const uc_hit *hits);
/* replace the engine's hit lists by the merge of n_parts shard lists (each: counts[n_seqs] + flat hits),
 * keeping per query the top max_seqs under the frozen order (score desc, target asc) */
int uc_engine_hits_merge(uc_engine *e, int n_parts, const uint32_t *const *counts, const uc_hit *const *hits);
/* the same merge as a free host function (needs no device): the post-exchange step of the multi-GPU
 * layout.  out_hits must hold out_capacity entries; *out_n receives the merged total. */
int uc_hits_merge(uint32_t n_seqs, int32_t max_seqs, int n_parts, const uint32_t *const *counts,
                  const uc_hit *const *hits, uint32_t *out_counts, uc_hit *out_hits, uint64_t out_capacity,
                  uint64_t *out_n);

/* ---- device-resident exchange for the multi-GPU layout: the hit lists never visit the host.
 * export: copy the engine's hit lists (hits_size elements per array, grouped by query) into caller-provided
 *         DEVICE buffers (e.g. the storage of a torch tensor that RCCL then all-gathers).
 * import: install the union of all shards' lists given as DEVICE arrays in any order: merge per query under the
 *         frozen order (score desc, target asc), keep max_seqs, and - if world > 1 - keep only the pairs owned by
 *         `rank`.  Ownership is a hash of the UNORDERED pair, so (q,t) and (t,q) land on the same rank and share
 *         their DP there; over all ranks every merged pair is aligned exactly once.  *n_kept = pairs installed. */
int uc_engine_hits_export_dev(const uc_engine *e, uint32_t *d_query, uint32_t *d_target, int32_t *d_score, int32_t *d_diag);
int uc_engine_hits_import_dev(uc_engine *e, uint64_t n, const uint32_t *d_query, const uint32_t *d_target, const int32_t *d_score,
                              const int32_t *d_diag, uint32_t rank, uint32_t world, uint64_t *n_kept);

/* ---- one process per GPU: the same sharded pass driven from outside (bench.py under torch.distributed.run) ----------
 * The data path stays inside the library: two ragged RCCL exchanges of the hit lists (grouped ncclSend / ncclRecv), device merges,
 * point-to-point edge gather.
 * Rank 0 creates an id and ships its 128 bytes to the other ranks by any means (a file, torch.distributed's store);
 * uc_comm_create is collective (ncclCommInitRank) and binds the communicator to HIP device `device`. */
typedef struct uc_comm uc_comm;
#define UC_COMM_ID_BYTES 128
int uc_comm_unique_id(uint8_t id[UC_COMM_ID_BYTES]);
int uc_comm_create(const uint8_t id[UC_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device, uc_comm **out);
void uc_comm_destroy(uc_comm *c);
/* what RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): the number of ranks
 * it was built over, this rank, its HIP device.  bench.py prints the count in its line; the N > 1 tests assert it == N. */
int uc_comm_info(const uc_comm *c, int32_t *nccl_ranks, int32_t *nccl_rank, int32_t *device);
/* One pass of the hot path on this rank: E1-E4 on the rank's cell of the Q x T grid (target_shards = T, 0 = one target
 * shard per GPU: the north-star layout) -> exchange 1 + merge at the home rank -> exchange 2 to the owner rank -> E5/E6 on the rank's pairs -> edges
 * to rank 0 -> set cover on rank 0.  comm == NULL runs the single-GPU pass.  assign[n_seqs] is written on rank 0 only
 * (may be NULL elsewhere); *n_alignments = gapped alignments of THIS rank. */
int uc_engine_cluster_step(uc_engine *e, uc_comm *comm, int32_t target_shards, uint32_t *assign, uint64_t *n_alignments);

/* E5-E6 for queries [qbegin,qend) of the engine's hit lists; results are kept per hit */
int uc_engine_align(uc_engine *e, uint32_t qbegin, uint32_t qend);
int uc_engine_alns_get(const uc_engine *e, uint32_t qbegin, uint32_t qend, uc_aln *out);   /* one per hit */
int uc_engine_edges_size(const uc_engine *e, uint64_t *n_edges);
int uc_engine_edges_get(const uc_engine *e, uint32_t *edges /* 2*n_edges: (query,target) */);

int uc_engine_stats(const uc_engine *e, uc_stats *out);
void uc_engine_reset_stats(uc_engine *e);
/* the prefilter's on-chip diagonal selection since the last reset: out[0] queries it took, out[1] queries of the double-hit path, out[2] surviving
 * keys it took, out[3] surviving keys (= n_filtered_hits of that path); UC_TD_ONCHIP=0 leaves [0] and [2] at 0 */
int uc_engine_td_onchip(const uc_engine *e, uint64_t *out /* 4 */);
/* the packed gapped kernel since the last reset: out[0] class launches in which a workgroup served several tasks (queries' pair lists), out[1] the
 * tasks of those launches; UC_SW_TASK_QUERIES=1 leaves both at 0.  Not part of uc_stats. */
int uc_engine_sw_task_queries(const uc_engine *e, uint64_t *out /* 2 */);

/* Kernel-level entry of the linear-time pre-step (E8a, uc_linclust.hip) on the engine's database; test support, uc_stats is untouched.
 * m <= 0: the engine's --kmer-per-seq, otherwise m in [1,1000] replaces it for this call.  install = 0: *n_out = number of sorted unique
 * (centre, member) pairs, copied to out_pairs[2 * i ..] when they fit into cap pairs (cap = 0: count only).  install = 1: the pairs become the
 * engine's hit lists (query = centre, score 0, diag 0; read them with uc_engine_hits_get), *n_out = their number, out_pairs is not written.
 * m > 1000, another install value or a missing pointer: UC_ERR_ARGS before the device is touched. */
int uc_engine_linclust_pairs(uc_engine *e, int32_t m, int32_t install, uint32_t *out_pairs, uint64_t cap, uint64_t *n_out);

/* E7 (host, as the north star prescribes): greedy set cover over (a,b) pairs; assign[i] = representative */
int uc_setcover(uint32_t n, const uint32_t *edges, uint64_t n_edges, uint32_t *assign);
/* the same result with the graph built on the engine's GPU (sort + unique of the edge list) and only the greedy
 * cover on the host: what uc_cluster and the bench step use */
int uc_engine_setcover(uc_engine *e, const uint32_t *edges, uint64_t n_edges, uint32_t *assign);
/* (ABI 9) E7 by clustering rule.  mode 0 = the greedy set cover (uc_setcover's result); mode 2 = greedy incremental (rule UC-1/G, what
 * `--cluster-mode 2` runs): the same undirected graph on the pairs, self loops and duplicates dropped; the nodes are walked by len descending (ties:
 * ascending id), an unassigned node becomes a representative and takes all its still-unassigned neighbours.  Any other mode is UC_ERR_ARGS.
 * uc_cluster_graph is the host variant (no device needed); len[n] = residue counts, may be NULL for mode 0. */
int uc_cluster_graph(uint32_t n, const uint32_t *edges, uint64_t n_edges, const uint32_t *len, int32_t mode, uint32_t *assign);
/* the device variant: n and the lengths are those of the engine's database; graph, rounds and assignment on the engine's GPU.  mode 0 gives
 * uc_engine_setcover's result. */
int uc_engine_cluster_graph(uc_engine *e, int32_t mode, const uint32_t *edges, uint64_t n_edges, uint32_t *assign);
/* Rule UC-1/R (`--cluster-reassign`) on the engine's resident database and its options, as uc_cluster runs it behind the last round of
 * the workflow.  assign_in[n] is an assignment with assign_in[assign_in[x]] == assign_in[x]; anything else (an entry out of range, a representative
 * that is itself a member) is UC_ERR_ARGS.  Every member is verified against its representative with the gapped stage (query = representative), the
 * rejected members are searched again against representatives + rejected members, and the engine's clustering rule (--cluster-mode) runs on the
 * graph of everything that was accepted: assign_out[n].  rejected_out (nullable): n flags, 1 = the member failed the verification.
 * counts = { members verified, rejected, accepted pairs of the re-search (self pairs not counted), final clusters }.  Adds an entry point only:
 * the ABI revision and uc_stats are unchanged. */
int uc_engine_reassign(uc_engine *e, const uint32_t *assign_in, uint32_t *assign_out, uint8_t *rejected_out, uint64_t counts[4]);
/* E8/E9 outputs from an assignment: cluster DB (<prefix>, .index, .dbtype) */
int uc_write_cluster_db(const char *out_cluster_db, uint32_t n, const uint32_t *assign);

/* ---- `unicore profile` (rule UC-P; /root/reference/src/modules/profile.rs:13-147): core genes of a clustering -------------
 * Map: <db>.map split on whitespace, field 0 a gene name, field 1 a species; a gene named on several lines belongs to every species listed
 * (a set); S = distinct species (profile.rs:20-29).  Rows: the TSV (clust.tsv or an .m8) split on whitespace, fields 0 (group name) and 1
 * (gene) are used; a group is a maximal run of consecutive rows with the same field 0 (profile.rs:55-77).  Per group, every row whose gene is
 * in the map adds 1 to cnt[s] and the gene to genes[s] for every species s of the gene (profile.rs:79-84); multiple = species with cnt >= 1,
 * single = species with cnt == 1 (profile.rs:121-122); the group is core iff single * 100 >= threshold * S in integers (profile.rs:134).
 * A core group's file lists `gene \t species` for every species with |genes[s]| == 1 (profile.rs:138-143: single counts rows, the file counts
 * distinct genes); full[s] = core groups with cnt[s] == 1 (profile.rs:60-71).
 * uc_profile_count (host, no device needed) and uc_profile_count_dev (the HIP kernels of uc_profile.hip on `device`, -1 = the current one)
 * take the same arrays and give the same outputs:
 *   group[n_rows]   dense group index of a row: starts at 0, never decreases, never skips, ends at n_groups - 1
 *   gene[n_rows]    gene id < n_genes, or UC_NO_GENE for a name that is not in the map
 *   sp_off[n_genes + 1], sp[]   gene -> species CSR, the ids of a gene distinct and ascending, each < n_species;
 *                   species ids are the rank of the species name in byte order
 *   single, multiple [n_groups], core [n_groups] (0 / 1), full [n_species]
 *   core_off [n_groups + 1], core_gene / core_species: the file lines of group g are core_off[g] .. core_off[g + 1], ascending species,
 *                   empty for a group that is not core; capacity = the number of (row, species) pairs
 * UC_ERR_ARGS: n_groups, n_genes or n_species >= 2^24, (row, species) pairs >= 2^32, a malformed group array, CSR or gene id. */
#define UC_NO_GENE 0xffffffffu
int uc_profile_count(uint64_t n_rows, const uint32_t *group, const uint32_t *gene, uint32_t n_groups, uint32_t n_genes, const uint64_t *sp_off,
                     const uint32_t *sp, uint32_t n_species, uint32_t threshold, uint32_t *single, uint32_t *multiple, uint8_t *core,
                     uint64_t *core_off, uint32_t *core_gene, uint32_t *core_species, uint32_t *full);
int uc_profile_count_dev(int32_t device, uint64_t n_rows, const uint32_t *group, const uint32_t *gene, uint32_t n_groups, uint32_t n_genes,
                         const uint64_t *sp_off, const uint32_t *sp, uint32_t n_species, uint32_t threshold, uint32_t *single, uint32_t *multiple,
                         uint8_t *core, uint64_t *core_off, uint32_t *core_gene, uint32_t *core_species, uint32_t *full);
/* == `unicore profile -t threshold <db_prefix> <tsv> <out_dir>` (profile.rs:149-172): reads <db_prefix>.map and the TSV (the database itself is
 * not opened), counts on o->device (UC_PROFILE_HOST=1, read per call: the host counter, no device needed), writes one <name>.txt per core group
 * (name = the group name's second `-`-separated field, else the whole name; a later group of the same name replaces the file), copiness.tsv
 * (always) and profile.chk ("0", then "1").  Lines inside a gene file and the warnings go by ascending species name in bytes (the reference
 * iterates hash maps).  o->verbosity is Unicore's own 0..4 scale here.  threshold > 100 is UC_ERR_ARGS, a map line with fewer than two fields
 * or a TSV row with fewer than two is UC_ERR_IO. */
int uc_profile(const char *db_prefix, const char *tsv, const char *out_dir, uint32_t threshold, const uc_opts *o);

/* ---- `unicore tree --no-inference` (rule UC-T; /root/reference/src/modules/tree.rs:17-137,299-331): a centre-star MSA of every core gene on
 * the engine's 3Di+AA gapped stage, filtered and concatenated.  Adds entry points only: the ABI revision and uc_stats are unchanged.
 * A *group* is one gene file, its *rows* the file's lines in order; grp_off[n_groups + 1] counts rows, every group has 1 .. 65535 of them.  Each
 * host function (no device needed) has a _dev sibling that runs the HIP kernels of uc_msa.hip on `device` (-1 = the current one) and gives the same
 * outputs byte for byte.
 * uc_msa_center (UC-T/C): scores holds, group after group, the packed upper triangle of the group's pair scores: m (m - 1) / 2 values, (i, j) with
 *   i < j at i m - i (i + 1) / 2 + (j - i - 1).  sum(i) = the sum over j != i of S(min, max) in 64 bits; centre[g] = the row with the largest sum,
 *   the earliest among equals (a group of one row: row 0).
 * uc_msa_star (UC-T/L and the rows): centre[g] is group-local.  res_off[n_rows + 1] / res0 / res1: the residues of every row as bytes, for n_tracks = 1
 *   or 2 tracks on the same offsets (track 0 is the amino acids: the column counts are taken from it).  Per row: aligned (0 = all gaps), qs / ts (start
 *   of the alignment in the centre / in the row) and the backtrace runs[run_off[r] .. run_off[r + 1]) as `length << 2 | op` (0 M, 1 I = centre residue
 *   only, 2 D = row residue only), centre as query; the centre's own entries are not read.  Slot s of a group (0 .. Lc, Lc = the centre's length) takes
 *   ins[s] = the longest D run any row emits after consuming exactly s centre residues (qs included); col[c] = c + ins[0] + .. + ins[c]; width = Lc +
 *   the sum of all ins; the insert block of slot s is the ins[s] columns before col[s] (the last ins[Lc] columns for s = Lc).  Cells start as '-';
 *   the centre's residue c goes to col[c], an M step at centre position c writes the row's residue at col[c], a D run is written left-justified
 *   into its slot's block, an I run writes nothing.  Outputs: width[n_groups]; col (Lc entries per group, back to back); cnt (per column: rows whose
 *   track-0 cell is not '-'; width[g] entries per group) within cnt_capacity; cells0 / cells1 (group g: m_g x width[g] bytes, row-major, back to
 *   back) within cells_capacity bytes each.  need_out (nullable, 2): the columns and the cell bytes the call needs, set as soon as the widths are
 *   known - also when a capacity is too small (UC_ERR_ARGS).  The centre lengths plus the lengths of all D runs bound the columns.
 *   UC_ERR_ARGS before the device is touched: a malformed grp_off / res_off / run_off, a centre outside its group, a word that is no run (op 3 or
 *   length 0), adjacent runs of one operation, a backtrace that overruns the centre or the row, 2^31 or more columns.
 * uc_msa_filter (UC-T/F, tree.rs:299-331): cells is one track as uc_msa_star lays it out.  Column c of group g is kept iff cnt * 100 >= threshold * m_g
 *   in integers (m_g counts every row).  keep (one flag per column), fwidth[n_groups], fcells (group g: m_g x fwidth[g], back to back; never more
 *   bytes than cells).  threshold > 100 is UC_ERR_ARGS. */
int uc_msa_center(uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, uint32_t *centre);
int uc_msa_center_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, uint32_t *centre);
int uc_msa_star(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, uint32_t n_tracks, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1,
                const int32_t *qs, const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, const uint8_t *aligned, uint32_t *width, uint32_t *col, uint32_t *cnt,
                uint64_t cnt_capacity, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out);
int uc_msa_star_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, uint32_t n_tracks, const uint64_t *res_off, const uint8_t *res0,
                    const uint8_t *res1, const int32_t *qs, const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, const uint8_t *aligned, uint32_t *width,
                    uint32_t *col, uint32_t *cnt, uint64_t cnt_capacity, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out);
int uc_msa_filter(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells, uint32_t threshold, uint8_t *keep, uint32_t *fwidth,
                  uint8_t *fcells);
int uc_msa_filter_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells, uint32_t threshold, uint8_t *keep,
                      uint32_t *fwidth, uint8_t *fcells);
/* == `unicore tree --no-inference -d threshold -o aligner_options <db_prefix> <profile_dir> <out_dir>` (tree.rs:17-137).  Reads <db>, <db>_ss, <db>_h and the
 * *.txt files of profile_dir (ascending file name; every line `gene species`, exactly two fields, the gene a name of <db>_h: anything else is UC_ERR_IO;
 * more than 65535 lines in a file is UC_ERR_ARGS).  Per gene file: the forward gapped score of every pair of rows (scores only) gives the centre; the
 * centre as query against every other row runs through the gapped stage as a `-a` search does, under
 * "-e 1e30 -c 0 --cov-mode 0 --min-seq-id 0 --rev-correction 0 --max-seqs 65535" followed by aligner_options (nullable; Foldseek-style flags, unknown
 * ones are UC_ERR_ARGS); a row the stage does not accept is all gaps.  Layout, rendering and filter run on o->device (UC_TREE_HOST=1, read per call:
 * the host twins; the DP needs the device either way).  Writes under out_dir: fasta/<gene>/aa.fasta, 3di.fasta (the rows as stored), <gene>.fa,
 * <gene>_3di.fa (the MSA, both tracks on the same columns), <gene>.fa.filtered; combined.fasta (names by first appearance over the kept genes, a gene
 * without the name contributes gaps), combined.fasta.partitions (`JTT+F+I+G, <gene>=<first>-<last>` per kept gene) and tree.chk ("0": inference is
 * what would set it to "1").  A gene that keeps no column is left out with a warning.  If out_dir/combined.fasta exists the call says so and returns
 * UC_OK without touching anything.  o->verbosity is Unicore's own 0..4 scale.  UC_TREE_BUDGET_BYTES (default 512 MiB) bounds the pairs of one scoring
 * batch and the cells of one layout call (whole groups; results do not depend on it); UC_TREE_DUMP=1 also writes fasta/<gene>/pair_scores.tsv. */
#define UC_TREE_NPHASE 7
typedef struct uc_tree_stats {
    uint64_t n_groups, n_rows;           /* gene files, their lines */
    uint64_t n_pairs_scored;             /* forward DPs of the all-pairs pass */
    uint64_t n_rows_unaligned;
    uint64_t n_columns, n_columns_kept;  /* before / after the filter, summed over the genes */
    uint64_t n_groups_dropped;           /* genes without a row or without a kept column */
    double seconds[UC_TREE_NPHASE];      /* host wall: [0] reading, [1] all-pairs scores, [2] centres, [3] centre alignments, [4] layout + render + filter,
                                            [5] writing, [6] the whole call */
} uc_tree_stats;
int uc_tree(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, const uc_opts *o,
            uc_tree_stats *stats_out);

/* ---- `unicore tree -a profile` (rule UC-T/P): profile refinement of the star MSA.  One round realigns every row of a group against the
 * leave-one-out column profile of the group's current MSA (one local affine DP over the full matrix, one walk), lays the rows out again by UC-T/L with a
 * virtual centre of the MSA's width and drops the columns without an amino acid.  Host functions need no device; the _dev siblings run the HIP kernels of
 * uc_msa_profile.hip and give the same bytes.  Track 0 is the amino acids, track 1 the 3Di letters, as in uc_msa_star.
 * uc_msa_profile_align: width[g] and cells0 / cells1 are the current MSA as uc_msa_star lays it out (group g: m_g x width[g] bytes); a cell is `-` or an
 *   ASCII letter (coded as the database loader codes it: ACDEFGHIKLMNPQRSTVWY -> 0 .. 19, any other letter 20), and both tracks hold their gaps in the
 *   same cells.  res_off / res0 / res1: the full rows as letters.  S3, SA: 21 x 21, [column letter][row letter].  Per row: aligned (score > 0), score,
 *   the first cell (qs = column, ts = residue), the end cell (qe, te; smallest te, then smallest qe) and the runs `length << 2 | op` (0 M, 1 I = column
 *   only, 2 D = residue only) at run_off[r] .. run_off[r + 1].  need_out (nullable) receives the run count; runs_capacity below it is UC_ERR_ARGS with
 *   run_off filled in.  width[g] + L_r words per row always suffice.  A group of one row is left alone: no DP runs, its row reports
 *   aligned = 0 without runs, and uc_msa_profile_layout keeps such a group's cells as they are.
 *   threads: host threads of the twin (0 = 1); the answer does not depend on it.
 * UC_ERR_ARGS: gap_open < gap_ext, gap_ext < 0 or gap_open > 2^20 (scores stay in 32 bits), a cell that is neither a letter nor `-`, tracks that
 *   disagree on a gap, width[g] * L_r >= 2^31, ceil(width[g] / chunk) * (L_r + chunk - 1) * chunk >= 2^31 (the decision bytes of the row as the kernel
 *   lays them out; both sides refuse it), more than 65534 rows in a group, malformed offsets.
 * uc_msa_profile_layout: the new MSA from the rows' alignments: ins[s], s = 0 .. width[g], = the longest D run after s columns, col[c] = c + sum of
 *   ins[0 .. c], M writes at col[c], D runs left-justified into their slot's block, I writes nothing, an unaligned row is all gaps; then every column
 *   without a residue on track 0 is dropped.  new_width [n_groups]; need_out[0] = cell bytes per track.  A group of one row keeps cells_in's row.
 * uc_msa_profile_geometry: chunk = columns of the MSA a wave stages in LDS at a time (wider tasks are served chunk after chunk: there is no cap on the
 *   width, *cap receives 0); task_bytes_per_cell = bytes of the decision buffer per DP cell. */
int uc_msa_profile_align(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0, const uint8_t *cells1, const uint64_t *res_off,
                         const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint8_t *aligned,
                         int32_t *score, int32_t *qs, int32_t *ts, int32_t *qe, int32_t *te, uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity,
                         uint64_t *need_out, uint32_t threads);
int uc_msa_profile_align_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0, const uint8_t *cells1,
                             const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int32_t gap_open,
                             int32_t gap_ext, uint8_t *aligned, int32_t *score, int32_t *qs, int32_t *ts, int32_t *qe, int32_t *te, uint64_t *run_off,
                             uint32_t *runs, uint64_t runs_capacity, uint64_t *need_out);
int uc_msa_profile_layout(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0_in, const uint8_t *cells1_in,
                          const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint8_t *aligned, const int32_t *qs, const int32_t *ts,
                          const uint64_t *run_off, const uint32_t *runs, uint32_t *new_width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity,
                          uint64_t *need_out);
int uc_msa_profile_layout_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0_in,
                              const uint8_t *cells1_in, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint8_t *aligned, const int32_t *qs,
                              const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, uint32_t *new_width, uint8_t *cells0, uint8_t *cells1,
                              uint64_t cells_capacity, uint64_t *need_out);
int uc_msa_profile_geometry(uint32_t *chunk, uint32_t *cap, uint32_t *task_bytes_per_cell);
/* == `unicore tree --no-inference -a profile --refine-iters refine_iters`: uc_tree, with refine_iters (0 .. UC_TREE_MAX_REFINE) rounds of UC-T/P between
 * the star MSA and the filter.  refine_iters = 0 writes exactly what uc_tree writes.  The rounds take the matrices and gaps of aligner_options, run on
 * o->device (UC_TREE_HOST=1: the host twins) in batches of tasks under UC_TREE_BUDGET_BYTES (no result depends on it); UC_TREE_DUMP=1 also writes
 * fasta/<gene>/refine.tsv (round, row, score, qs, ts). */
#define UC_TREE_MAX_REFINE 8
#define UC_TREE_REFINED_NPHASE 3
typedef struct uc_tree_refined_stats {
    uc_tree_stats tree;                  /* of the whole call; n_rows_unaligned counts the rows that are all gaps in the final MSA */
    uint64_t n_rounds, n_tasks, n_cells; /* rounds run; DPs (rows of groups with two rows or more, summed over the rounds); their cells, width x length */
    uint64_t n_rows_became_aligned, n_rows_became_unaligned;      /* against the MSA the round started from, summed over the rounds */
    uint64_t width_before[UC_TREE_MAX_REFINE], width_after[UC_TREE_MAX_REFINE];      /* per round, summed over the genes */
    double seconds[UC_TREE_REFINED_NPHASE];      /* host wall: [0] profile DP + walk, [1] layout + compaction, [2] both */
} uc_tree_refined_stats;
int uc_tree_refined(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, uint32_t refine_iters,
                    const uc_opts *o, uc_tree_refined_stats *stats_out);

/* ---- `unicore tree -a progressive` (rule UC-T/G): a progressive MSA.  The rows of a group are merged along a guide tree by
 * profile-profile alignment; no residue is dropped and no column is empty.  Host functions need no device; the _dev siblings run the HIP kernels of
 * uc_msa_progressive.hip and give the same bytes.  Track 0 is the amino acids, track 1 the 3Di letters; letters are coded as in uc_msa_profile_align.
 * S3, SA: 21 x 21 within -48 .. 48, [column letter][row letter], side a giving the column letter.  UC_ERR_ARGS everywhere: gap_open < gap_ext or
 * gap_ext < 0, a group of more than 8192 rows, malformed offsets, a matrix entry outside -48 .. 48.
 * uc_msa_self_scores: self[r] = sum over the row's residues of SA[a][a] + S3[d][d].
 * uc_msa_guide (UC-T/G/T): scores as uc_msa_center takes them (row i as query), self per row.  D receives, group after group, m x m doubles:
 *   den = min(self(i), self(j)); D = 1 where den <= 0, else 1 - (double)S / (double)den, clamped below at 0.  merges receives m - 1 pairs (a, b) of
 *   group-local node ids per group, group g's at word 2 (grp_off[g] - g): the records of uc_nj_join over D in order (join_a is the a side; record k
 *   creates node m + k), then (root_node[0], root_node[1]), then (that node, root_node[2]).  m = 2: (0, 1) without the join; m = 1: nothing.  The _dev
 *   sibling runs uc_nj_join_dev for groups of 256 rows or more; the join is bit-identical, so no result depends on it.
 * uc_msa_merge (UC-T/G/M): n_tasks independent merges.  Task k joins a (ma x Wa) with b (mb x Wb); a0 / a1 (b0 / b1) hold the sides' cells on the two
 *   tracks, task after task, m x W bytes row-major; a cell is `-` or a letter and the tracks agree on gaps.  Per track cnt[column][letter] counts a
 *   side's rows; s(i, j) = floor(sum over tracks, x, y of cntA[i][x] cntB[j][y] S[x][y] / (ma mb)).  H(i, 0) = H(0, j) = 0, E = F = -2^28 on the
 *   borders; H = max(H(i-1, j-1) + s, F, E) without a floor at 0, F(i, j) = max(H(i-1, j) - open, F(i-1, j) - ext) (a's column alone, op I),
 *   E(i, j) = max(H(i, j-1) - open, E(i, j-1) - ext) (b's column alone, op D).  The end cell (ie, je) is taken over i = Wa or j = Wb, the corners
 *   (Wa, 0) and (0, Wb) included: largest H, then smallest j, then smallest i.  The walk (E6's preferences) ends at (is, js), one of them 0; runs are
 *   `length << 2 | op` (0 M, 1 I, 2 D) at run_off[k] .. run_off[k + 1].  The merged node, (ma + mb) x width[k] with a's rows first, at cells0 / cells1,
 *   tasks back to back: a[0 .. is) or b[0 .. js), the path, a[ie .. Wa) or b[je .. Wb).  A side of width 0: no DP, score and positions 0, the other
 *   side's columns.  need_out[2] (nullable): runs and cell bytes per track; Wa + Wb words and (ma + mb) (Wa + Wb) bytes per task always suffice.
 *   UC_ERR_ARGS also: ma or mb 0, ma + mb > 8192, Wa Wb >= 2^31, (Wa + Wb) max(open, 96) >= 2^27, ceil(Wa / chunk) (Wb + chunk - 1) chunk >= 2^31
 *   (the score and decision bytes of a task as the kernels lay them out, an implementation limit on top of the rule's two; the twin refuses it too).
 * uc_msa_progressive: the MSA of every group along its merge list (laid out as uc_msa_guide writes it; taken as an input, so that a caller may force a
 *   tree).  A leaf is its row's residues.  Merges run by level: a level is every merge whose two children exist.  width[g] and group g's m_g x width[g]
 *   cells, rows in file order.  The sum of a group's residues times its rows always suffices as capacity.  UC_ERR_ARGS also: a merge list that is not a
 *   tree over the group (a child that does not exist yet or is used twice); a merge whose two sides, at the widths they have when their level is reached,
 *   break the width limits of uc_msa_merge (checked on the host before the level runs, by twin and device alike).
 * uc_msa_progressive_geometry: chunk = a's columns a wave holds at a time (wider tasks run chunk after chunk, *cap receives 0); task_bytes_per_cell =
 *   bytes of the score and decision buffers per DP cell. */
typedef struct uc_msa_progressive_stats {
    uint64_t n_merges, n_levels;         /* merges run; levels over all groups of the call */
    uint64_t n_launches;                 /* kernel launches of the device side (0 from the host twin): 5 per batch of a level, beside one rocPRIM scan */
    uint64_t n_cells;                    /* DP cells, Wa x Wb summed over the merges */
} uc_msa_progressive_stats;
int uc_msa_self_scores(uint64_t n_rows, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int64_t *self);
int uc_msa_guide(uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, const int64_t *self, double *D, uint32_t *merges);
int uc_msa_guide_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, const int64_t *self, double *D, uint32_t *merges);
int uc_msa_merge(uint32_t n_tasks, const uint32_t *ma, const uint32_t *mb, const uint32_t *Wa, const uint32_t *Wb, const uint8_t *a0, const uint8_t *a1, const uint8_t *b0,
                 const uint8_t *b1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, int32_t *score, int32_t *is, int32_t *js, int32_t *ie, int32_t *je,
                 uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out,
                 uint32_t threads);
int uc_msa_merge_dev(int32_t device, uint32_t n_tasks, const uint32_t *ma, const uint32_t *mb, const uint32_t *Wa, const uint32_t *Wb, const uint8_t *a0, const uint8_t *a1,
                     const uint8_t *b0, const uint8_t *b1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, int32_t *score, int32_t *is, int32_t *js, int32_t *ie,
                     int32_t *je, uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity,
                     uint64_t *need_out);
int uc_msa_progressive(uint32_t n_groups, const uint64_t *grp_off, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint32_t *merges, const int8_t *S3,
                       const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out,
                       uc_msa_progressive_stats *stats_out, uint32_t threads);
int uc_msa_progressive_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint32_t *merges,
                           const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity,
                           uint64_t *need_out, uc_msa_progressive_stats *stats_out);
int uc_msa_progressive_geometry(uint32_t *chunk, uint32_t *cap, uint32_t *task_bytes_per_cell);
/* == `unicore tree --no-inference -a progressive`: uc_tree with the progressive MSA in the star MSA's place.  The all-pairs scores are the pass uc_tree
 * runs for its centres; self scores, D, the guide trees (UC-N/J) and the merges follow; filter, concatenation and files are uc_tree's.  The merges take
 * the matrices and gaps of aligner_options (gap open >= gap extension >= 0) and run on o->device level by level over all genes, in batches of whole
 * tasks under UC_TREE_BUDGET_BYTES (no result depends on it); UC_TREE_HOST=1 runs the host twins (the pair scores need the device either way);
 * UC_TREE_DUMP=1 also writes fasta/<gene>/guide.tsv: a line `#D\ti\tj\t%.17g` per pair, then a line `k\ta\tb` per merge. */
#define UC_TREE_PROGRESSIVE_NPHASE 3
typedef struct uc_tree_progressive_stats {
    uc_tree_stats tree;                  /* of the whole call; n_rows_unaligned is 0: every residue is in the MSA */
    uint64_t n_groups_aligned;           /* genes with a row */
    uint64_t n_merges, n_levels, n_launches, n_cells;      /* as uc_msa_progressive_stats; a caterpillar tree of m rows gives m - 1 levels */
    uint64_t width_before, width_after;  /* root widths summed over the genes, before and after the filter */
    double seconds[UC_TREE_PROGRESSIVE_NPHASE];      /* host wall: [0] self scores + guide trees, [1] merges, [2] both */
} uc_tree_progressive_stats;
int uc_tree_progressive(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, const uc_opts *o,
                        uc_tree_progressive_stats *stats_out);

/* ---- the built-in tree builder `nj` (rule UC-N): pairwise protein distances over an aligned FASTA and neighbour joining (Saitou-Nei
 * with the Studier-Keppler criterion), the inference step of `unicore tree -t nj` and `unicore gene-tree -t nj` (tree.rs:139-161 and genetree.rs hand it
 * to an external program).  Every output is defined bit for bit; every host function (no device needed) has a _dev sibling that runs the HIP kernels
 * of uc_nj.hip on `device` (-1 = the current one) and gives the same integers and the same fp64 bits.  Limits, all UC_ERR_ARGS before the device is
 * touched: 2 <= n <= 16384, 1 <= w < 2^31.
 * uc_nj_counts (UC-N/D): cells is n rows of w bytes, row-major.  A cell is informative iff it is an ASCII letter other than X / x; letters compare
 *   case-insensitively.  comp / diff [n (n - 1) / 2], (i, j) with i < j at i n - i (i + 1) / 2 + (j - i - 1): the columns where both cells are
 *   informative, and those of them where the letters differ.  threads: host threads of the host twin (0 = 1); the device side reads
 *   UC_TREE_BUDGET_BYTES (default 512 MiB) per call and serves n x w beyond it in column slices (results do not depend on it).
 * uc_nj_distances: p = diff / comp; model 0 (kimura): t = 1 - p - 0.2 p p, d = 5 if comp == 0 or t <= 0, else min(5, -log(t)); model 1 (p): d = p, or 5
 *   if comp == 0.  D [n x n] fp64, symmetric, 0 on the diagonal.
 * uc_nj_join (UC-N/J): D is not modified.  join_a / join_b / len_a / len_b [n - 3]: step s joins the nodes in slots i < j (leaves are nodes 0 .. n - 1,
 *   step s creates node n + s) at lengths len_a / len_b; root_node / root_len [3]: the trifurcation (n == 2: both leaves at half their distance, the
 *   third entry UC_NJ_NO_NODE / 0).  No length is negative or -0.0.
 * uc_nj_newick: names [n] NUL-terminated; one line `(A:la,B:lb,C:lc);\n`, children in record order, lengths %.6f, a name holding any of ()[]:;,' or
 *   white space in single quotes with ' doubled.  need (optional) receives the length without the NUL; buf may be NULL with cap 0 to ask for it; a
 *   buffer that is too small (cap < need + 1) is UC_ERR_ARGS.
 * uc_nj_geometry: the tile height (rows) and the LDS column chunk of the count kernel. */
#define UC_NJ_NO_NODE 0xffffffffu
#define UC_NJ_MODEL_KIMURA 0
#define UC_NJ_MODEL_P 1
int uc_nj_counts(uint32_t n, uint64_t w, const uint8_t *cells, uint32_t threads, uint32_t *comp, uint32_t *diff);
int uc_nj_counts_dev(int32_t device, uint32_t n, uint64_t w, const uint8_t *cells, uint32_t threads, uint32_t *comp, uint32_t *diff);
int uc_nj_distances(const uint32_t *comp, const uint32_t *diff, uint32_t n, uint32_t model, double *D);
int uc_nj_join(uint32_t n, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node, double *root_len);
int uc_nj_join_dev(int32_t device, uint32_t n, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node,
                   double *root_len);
int uc_nj_newick(const char *const *names, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, const double *len_a, const double *len_b,
                 const uint32_t *root_node, const double *root_len, char *buf, uint64_t cap, uint64_t *need);
int uc_nj_geometry(uint32_t *tile_rows, uint32_t *chunk_columns);
/* == the inference step of `unicore tree -t nj`: reads the aligned FASTA msa_fasta (any line wrapping; a name ends at the first white space; a duplicate
 * or empty name is UC_ERR_IO; rows of unequal width are UC_ERR_ARGS), counts on o->device, transforms under `model` ("kimura", "p"; NULL = kimura;
 * anything else UC_ERR_ARGS), joins and writes the Newick line to out_nwk.  UC_TREE_HOST=1 (read per call) runs the host twins and needs no GPU;
 * UC_TREE_DUMP=1 also writes <out_nwk>.dist.tsv (i, j, comp, diff, d as %.17g).  o->verbosity is Unicore's own 0..4 scale. */
#define UC_NJ_NPHASE 5
typedef struct uc_nj_stats {
    uint64_t n_rows, n_columns;
    uint64_t n_pairs_incomparable;       /* comp == 0 */
    uint64_t n_pairs_capped;             /* d == 5.0 */
    uint64_t n_lengths_clamped;          /* branch lengths stored as 0 */
    double seconds[UC_NJ_NPHASE];        /* host wall: [0] reading, [1] counts, [2] transform, [3] joins, [4] writing */
} uc_nj_stats;
int uc_tree_infer(const char *msa_fasta, const char *out_nwk, const char *model, const uc_opts *o, uc_nj_stats *stats_out);

/* ---- bootstrap support for `nj` (rule UC-N/B): B replicate trees over columns drawn with replacement, and for every internal branch
 * of the main tree the number of replicates that hold the same split.  The reference's `iqtree -B 1000` (tree.rs:139-161) labels its tree the same way.
 * Every output is defined bit for bit; the _dev siblings run the HIP kernels of uc_nj_boot.hip with the replicate as a grid dimension.  Limits, all
 * UC_ERR_ARGS before the device is touched: those of UC-N, and rep0 + n_rep <= 100000.
 * Draws, modulo 2^64 with G = 0x9E3779B97F4A7C15 and mix = SplitMix64's finaliser: key = mix(seed + G (rep + 1)), x = mix(key + G (t + 1)), column t of
 *   replicate rep is source column (x w) >> 64.  The host-only column entry point writes the w draws of one replicate.
 * Replicate counts: comp / diff [n_rep][n (n - 1) / 2] of replicates rep0 .. rep0 + n_rep - 1: UC-N/D over the drawn columns.  The device side works
 *   under UC_TREE_BUDGET_BYTES in batches of replicates and slices of source columns; no result depends on it.
 * Batched joins: D [n_rep][n][n] (not modified); every output array is the single call's, replicate after replicate ([n_rep][n - 3], [n_rep][3]), and
 *   equals UC-N/J on D[b] by bits.  n <= lds_rows of the geometry call runs one workgroup per replicate with D in LDS, larger n three launches per step
 *   for the whole batch.
 * Support: join s of the main tree creates node n + s; its split is {the leaves below it, the others}.  support [n - 3] receives the number of
 *   replicates (join_a / join_b [n_rep][n - 3]) with the same split, compared as leaf sets.  n <= 3 writes nothing.
 * Labelled Newick: the unlabelled line with (200 support[s] + n_rep) div (2 n_rep) - the percentage, rounded half up - between the `)` of node n + s and
 *   its `:`; the root has no label; n_rep == 0 (support may be NULL) gives the unlabelled line. */
int uc_nj_boot_columns(uint64_t w, uint64_t seed, uint32_t rep, uint32_t *cols);
int uc_nj_boot_counts(uint32_t n, uint64_t w, const uint8_t *cells, uint64_t seed, uint32_t rep0, uint32_t n_rep, uint32_t threads, uint32_t *comp,
                      uint32_t *diff);
int uc_nj_boot_counts_dev(int32_t device, uint32_t n, uint64_t w, const uint8_t *cells, uint64_t seed, uint32_t rep0, uint32_t n_rep, uint32_t threads,
                          uint32_t *comp, uint32_t *diff);
int uc_nj_join_batch(uint32_t n, uint32_t n_rep, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node,
                     double *root_len);
int uc_nj_join_batch_dev(int32_t device, uint32_t n, uint32_t n_rep, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b,
                         uint32_t *root_node, double *root_len);
int uc_nj_support(uint32_t n, const uint32_t *join_a, const uint32_t *join_b, uint32_t n_rep, const uint32_t *rep_join_a, const uint32_t *rep_join_b,
                  uint32_t *support);
int uc_nj_newick_support(const char *const *names, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, const double *len_a, const double *len_b,
                         const uint32_t *root_node, const double *root_len, const uint32_t *support, uint32_t n_rep, char *buf, uint64_t cap,
                         uint64_t *need);
int uc_nj_boot_geometry(uint32_t *lds_rows);
/* == `unicore tree -t nj -p "--bootstrap B --seed S"`: the main tree as the plain inference call computes it (unchanged in every bit), n_rep replicate
 * trees, and out_nwk with the labels.  n_rep == 0 writes what the plain call writes.  UC_TREE_HOST=1 and UC_TREE_DUMP=1 as there; a dump with
 * n_rep > 0 also writes <out_nwk>.boot.tsv (one line `s\tsupport` per join) and <out_nwk>.boottrees (the replicates' unlabelled lines, in order). */
#define UC_NJ_BOOT_NPHASE 7
typedef struct uc_nj_boot_stats {
    uint64_t n_rows, n_columns, n_replicates;
    uint64_t n_batches;                  /* batches of replicates the budget gave */
    uint64_t support_min, support_sum;   /* over the n - 3 joins; 0 without an internal branch */
    double seconds[UC_NJ_BOOT_NPHASE];   /* host wall: [0] reading, [1] main tree, [2] draws + counts, [3] transform, [4] joins, [5] support, [6] writing */
} uc_nj_boot_stats;
int uc_tree_infer_boot(const char *msa_fasta, const char *out_nwk, const char *model, uint32_t n_rep, uint64_t seed, const uc_opts *o,
                       uc_nj_boot_stats *stats_out);

/* ---- transfer bootstrap support for `nj` (rule UC-N/T; TBE, Lemoine et al., Nature 2018): for a branch of the main tree and a
 * replicate tree, the fewest leaves that would have to move for the branch to appear, averaged over the replicates.  Integers throughout; the _dev
 * sibling runs the HIP kernels of uc_nj_transfer.hip.  Limits, all UC_ERR_ARGS before the device is touched: those of UC-N and UC-N/B, and join records
 * that do not form a tree (a node joined twice or before it exists), the main tree's or a replicate's.
 * Join s of a tree on n leaves creates node n + s with leaf set L_s; light[s] = min(|L_s|, n - |L_s|) >= 2.  For a main split x and a replicate split y,
 *   h = popcount(x xor y) over the n-bit sets and delta = min(h, n - h).  phi[b][s] = min(light[s] - 1, min over replicate b's n - 3 joins of delta): the
 *   cap is what the replicate's terminal branches would give.  phi[b][s] == 0 exactly when replicate b holds the split (uc_nj_support counts those).
 * uc_nj_transfer: phi [n_rep][n - 3] and light [n - 3]; threads: host threads of the twin (0 = 1), replicates spread over them.  n <= 3 writes
 *   nothing.  The device side works under UC_TREE_BUDGET_BYTES in batches of replicates; no result depends on it.
 * Labelled Newick: phi_sum[s] = the sum of phi[b][s] over the replicates (64 bits), den = n_rep (light[s] - 1), the label of node n + s is the
 *   percentage of 1 - phi_sum[s] / den rounded half up, (200 (den - phi_sum[s]) + den) div (2 den); phi_sum[s] > den is UC_ERR_ARGS; n_rep == 0 (light and
 *   phi_sum may be NULL) gives the unlabelled line.
 * uc_nj_transfer_geometry: the splits of a tile of the comparison kernel, the 32-bit words of a split staged through LDS at a time, and the largest
 *   tree for which uc_tree_infer_support runs the twin also on a device run (the device call's fixed cost is above the twin's whole time there). */
#define UC_NJ_SUPPORT_FBP 0
#define UC_NJ_SUPPORT_TBE 1
int uc_nj_transfer(uint32_t n, const uint32_t *join_a, const uint32_t *join_b, uint32_t n_rep, const uint32_t *rep_join_a, const uint32_t *rep_join_b,
                   uint32_t threads, uint32_t *phi, uint32_t *light);
int uc_nj_transfer_dev(int32_t device, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, uint32_t n_rep, const uint32_t *rep_join_a,
                       const uint32_t *rep_join_b, uint32_t threads, uint32_t *phi, uint32_t *light);
int uc_nj_newick_transfer(const char *const *names, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, const double *len_a, const double *len_b,
                          const uint32_t *root_node, const double *root_len, const uint32_t *light, const uint64_t *phi_sum, uint32_t n_rep, char *buf,
                          uint64_t cap, uint64_t *need);
int uc_nj_transfer_geometry(uint32_t *tile_splits, uint32_t *chunk_words, uint32_t *host_leaves);
/* == `unicore tree -t nj -p "--bootstrap B --support fbp|tbe"`: uc_tree_infer_boot with the support rule as an argument.  UC_NJ_SUPPORT_FBP is that
 * call, byte for byte; UC_NJ_SUPPORT_TBE labels the same main tree with UC-N/T's percentages, reports the transfer time in seconds[5], keeps
 * support_min / support_sum as the counts of replicates that hold a split (the zeros of phi), and a dump's <out_nwk>.boot.tsv reads
 * `s\tsupport\tlight\tphi_sum\tlabel`.  Any other mode is UC_ERR_ARGS before a file is read. */
int uc_tree_infer_support(const char *msa_fasta, const char *out_nwk, const char *model, uint32_t n_rep, uint64_t seed, uint32_t support_mode,
                          const uc_opts *o, uc_nj_boot_stats *stats_out);

/* ---- kernel-level entry points (parity tests call the HIP kernels through these) -------------- */
/* ungapped diagonal score (E3) for n candidates (q[i], t[i], diag[i]) of the engine's DB */
int uc_engine_ungapped_batch(uc_engine *e, uint64_t n, const uint32_t *q, const uint32_t *t,
                             const int32_t *diag, int32_t *score_out);
/* E3 and the key pass of E4 for n candidates, with the prefilter's own launches: the scores (score_out may be null), the overlap residues
 * E3 counts for the stage's algorithmic bytes, and the number of candidates with score >= min_score that E4 keeps */
int uc_engine_ungapped_select(uc_engine *e, uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *diag, int32_t min_score,
                              int32_t *score_out, uint64_t *overlap_out, uint64_t *kept_out);
/* rule UC-1/X (--prefilter-mode 1) for queries [qbegin, qend) x targets [tbegin, tend) of the engine's DB: dense row-major
 * [qend - qbegin][tend - tbegin] arrays, the best ungapped score over ALL diagonals (capped at 255) and the smallest diagonal that
 * reaches it.  Computed tile by tile under tile_bytes (0 = the engine's default tile budget). */
int uc_engine_ungapped_all(uc_engine *e, uint32_t qbegin, uint32_t qend, uint32_t tbegin, uint32_t tend, uint64_t tile_bytes,
                           int32_t *score_out, int32_t *diag_out);
/* gapped DP (E5) for n pairs.  mode 0: forward (score, qend, tend); mode 1: reversed query (score);
 * mode 2: start pass on reverse(q[0..qend_in]) x reverse(t[0..tend_in]) (score, qend', tend').
 * Pairs may be in any order (the engine groups them by query internally). */
int uc_engine_sw_batch(uc_engine *e, int mode, uint64_t n, const uint32_t *q, const uint32_t *t,
                       const int32_t *qend_in, const int32_t *tend_in,
                       int32_t *score_out, int32_t *qend_out, int32_t *tend_out);
/* ONE pass of the gapped stage on n pairs, as Engine::align runs it: class table `table` (0: int32, 1: packed, 2: int32 traceback
 * statistics, 3: packed sparse) and mode - table 0: 0, 1, 2;  1: 0, 1, 2, 4, 6, 7;  2: 3;  3: 4, 6 (4 / 6: modes 0 / 2 with the optimum
 * known; 7: traceback bytes + walk).  box [n][4] = (qs, qe, ts, te): modes 2 / 6 read qe, te (forward end), modes 3 / 7 the whole box;
 * known [n] (> 0): modes 4, 6, 7 (7: the box's score).  band: half-width W of the stored band of mode 7 (0 = whole box).
 * raw = 1: the kernels' outputs as they are (packed: qend -2 for an ambiguous end row, scores >= the packed range limit; mode 7: pairs
 * whose walk left the band keep aln_len = idents = gaps = -1).  raw = 0: the library's re-run rules (int32 re-runs, mode 7 scores beyond
 * the packed range in int32 mode 3, band misses with the whole box).  Outputs (any may be NULL): score, qend, tend (modes 0 / 2 / 4 / 6;
 * tend keeps the one-row bit 1 << 30 of mode 6), class (the table's class of the pair, its class count = long-query kernel),
 * aln_len / idents / gaps (modes 3 / 7), miss (mode 7, band > 0: the walk left the band).  Anything else is UC_ERR_ARGS. */
int uc_engine_sw_pass(uc_engine *e, int table, int mode, int band, int raw, uint64_t n, const uint32_t *q, const uint32_t *t,
                      const int32_t *box, const int32_t *known, int32_t *score_out, int32_t *qend_out, int32_t *tend_out,
                      int32_t *class_out, int32_t *aln_len_out, int32_t *idents_out, int32_t *gaps_out, int32_t *miss_out);
/* (ABI 8) uc_engine_sw_pass with the second answer of the known-score modes 4 / 6 (anything else with a non-NULL qend2_out / tend2_out is
 * UC_ERR_ARGS).  Among several optimal cells the pass reports the one in the first optimal column, then the first row (qend_out, tend_out); the
 * second answer is the one in the first optimal ROW, then the first column - what the same pass reports for the pair (t, q) with the roles
 * swapped, since the two DPs are transposes of each other (symmetric matrices).  The gapped stage uses it to serve both directions of a mutual
 * hit from one DP.  -2 / -2 for a pair whose result did not come from the packed known-score kernel (queries beyond the systolic classes, and
 * with raw = 0 the int32 re-runs).  Mode 6 reports it relative to the box like qend_out / tend_out. */
int uc_engine_sw_pass2(uc_engine *e, int table, int mode, int band, int raw, uint64_t n, const uint32_t *q, const uint32_t *t,
                       const int32_t *box, const int32_t *known, int32_t *score_out, int32_t *qend_out, int32_t *tend_out,
                       int32_t *class_out, int32_t *aln_len_out, int32_t *idents_out, int32_t *gaps_out, int32_t *miss_out,
                       int32_t *qend2_out, int32_t *tend2_out);

/* ---- alignment backtraces (-a; ABI 7).  A backtrace is a slice of runs, each `length << 2 | op` with op 0 = M (diagonal step, match or
 * mismatch), 1 = I (query residue only), 2 = D (target residue only), from the start of the alignment to its end; adjacent runs differ in op.
 * An engine created with -a in its options keeps them on the device for every hit uc_engine_align accepts.
 * uc_engine_backtraces_get is aligned with uc_engine_alns_get: run_off holds one entry per hit of the query range plus one, slice k is
 * runs[run_off[k] .. run_off[k + 1]), empty for hits that were not accepted.  uc_engine_backtraces_size gives the length of `runs`. */
int uc_engine_backtraces_size(const uc_engine *e, uint32_t qbegin, uint32_t qend, uint64_t *n_runs);
int uc_engine_backtraces_get(const uc_engine *e, uint32_t qbegin, uint32_t qend, uint64_t *run_off, uint32_t *runs);
/* A slice as text ("35M2D110M1I7M"), NUL-terminated, as uc_search -a writes it into the 15th field of an alignment-DB row and
 * uc_convertalis prints it in its `cigar` column.  len_out (optional) receives the length without the NUL; a buffer that is too
 * small and a word that is no run are UC_ERR_ARGS. */
int uc_backtrace_render(const uint32_t *runs, uint64_t n_runs, char *out, uint64_t out_capacity, uint64_t *len_out);
/* uc_convertalis reads `--format-output LIST` from uc_opts.cluster_options (comma-separated column names; default: the 12 BLAST-tab
 * columns).  This checks a LIST the same way: UC_OK and the number of columns, or UC_ERR_ARGS for an unknown name. */
int uc_format_output_check(const char *list, uint32_t *n_columns);
/* Kernel-level sibling of uc_engine_sw_pass: ONE traceback pass with emission on the n boxes box[4 i ..] = (qs, qe, ts, te), raw (no redo
 * of band misses), by route: 0 = table 1 MODE 7 + walk with half band `band`, 1 = the same with the whole box stored, 2 = the stored
 * int32 matrix for every pair (the route of scores beyond the packed range and of the all-int32 configuration), 3 = the long-query route
 * of the packed pass (every query must be longer than the systolic classes; routes 0 / 1 take only shorter ones).  known[i] = the
 * box's optimum score (routes 0, 1, 3).  Outputs in list order, any may be NULL except run_off (n + 1): class of table 1, statistics,
 * band-miss mark, plain_out = 1 where the stored-int32-matrix kernels served the pair, and the slices (empty for a band miss).
 * More runs than runs_capacity is UC_ERR_ARGS with the number needed in *n_runs. */
int uc_engine_tb_emit_pass(uc_engine *e, int route, int band, uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *box, const int32_t *known,
                           int32_t *class_out, int32_t *aln_len_out, int32_t *idents_out, int32_t *gaps_out, int32_t *miss_out, int32_t *plain_out,
                           uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint64_t *n_runs);

/* ---- kernel-level entry points of the ProstT5 encoder (tests/test_t5_kernels.py calls the HIP kernels through these).
 * Each device call takes host arrays: it allocates, copies, runs the library's own launcher on `device` (-1 = the current one),
 * synchronizes, copies back and frees.  Inputs that break a kernel's preconditions are UC_ERR_ARGS before the device is touched.
 * f16 data crosses as uint16_t bit patterns.
 * uc_t5_gemm_variant (host only): the kernel the encoder's GEMM picks for M x N x K: 0 = 128 x 128 tile, 1 = 256 x 256 tile,
 *   2 = 256 x 256 two-phase persistent.  Every shape needs K % 64 == 0 and N % 4 == 0.
 * uc_t5_kernel_gemm: out[M, N] (+)= A[M, K] . W[N, K]^T; epi 0: f16 out, 1: ReLU + f16 out, 2: fp32 out, read and accumulated into.
 *   variant -1 = the library's pick; a forced variant must admit the shape (1: N % 256 == 0; 2: also K >= 128 and M * K, N * K < 2^31).
 * uc_t5_kernel_rmsnorm: y[T, D] (f16) = x * rsqrt(mean(x^2) + eps) * w, x fp32 [T, D], w fp32 [D]; D % 4 == 0.
 * uc_t5_kernel_attention: n_seqs sequences of seq_len[i] tokens packed in order; qkv [T, 3 * H * 128] (q | k | v), out [T, H * 128];
 *   bias [H][2 * bias_span - 1] fp32 indexed by key - query + bias_span - 1; bias_span >= max seq_len.
 * uc_t5_kernel_cnn_head: seq_len[i] counts a sequence's tokens including <AA2fold> and </s> (>= 2); x [T, D] f16 (D % 64 == 0);
 *   w1 [C1][D][KW], b1 [C1], w2 [NO][C1][KW], b2 [NO] fp32 (GGUF order; w1 is rounded to f16 as the loader does); KW odd <= 31,
 *   NO <= 21.  The conv1 GEMM plus the head kernels; codes [T], logits [T, NO] (nullable) are written for every token.
 * uc_t5_bias_table (host only): the table the encoder uploads, rel_bias [H][buckets] -> out [H][2 * span - 1]. */
int uc_t5_gemm_variant(int32_t M, int32_t N, int32_t K, int32_t *variant);
int uc_t5_kernel_gemm(int32_t device, int32_t variant, int32_t epi, int32_t M, int32_t N, int32_t K, const uint16_t *A, const uint16_t *W, void *out);
int uc_t5_kernel_rmsnorm(int32_t device, int32_t T, int32_t D, float eps, const float *x, const float *w, uint16_t *y);
int uc_t5_kernel_attention(int32_t device, int32_t H, int32_t n_seqs, const int32_t *seq_len, int32_t bias_span, const float *bias,
                           const uint16_t *qkv, uint16_t *out);
int uc_t5_kernel_cnn_head(int32_t device, int32_t n_seqs, const int32_t *seq_len, int32_t D, int32_t C1, int32_t KW, int32_t NO, int32_t eos_in_head,
                          const uint16_t *x, const float *w1, const float *b1, const float *w2, const float *b2, uint8_t *codes, float *logits);
int uc_t5_bias_table(int32_t H, int32_t buckets, int32_t max_dist, int32_t span, const float *rel_bias, float *out);

#ifdef __cplusplus
}
#endif
#endif
