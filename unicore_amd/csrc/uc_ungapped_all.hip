// uc_ungapped_all.hip — rule UC-1/X (--prefilter-mode 1): the exhaustive ungapped prefilter.  Every query of a batch against every target of a
// chunk, all diagonals: the pair's score is the best E3 score over the diagonals -(Lt-1) .. Lq-1 (capped at 255), its diagonal the smallest one
// that reaches it.  One kernel fills a (query batch x target chunk) tile of scores (one byte per pair) and diagonals; a second one turns the
// pairs that pass --min-ungapped-score into the candidate arrays the E4 selection of the k-mer path takes (uc_hit_lists.hip; the tile loop: uc_prefilter.hip).
//
// The scan.  A LANE OWNS A DIAGONAL: lane l of a wave works on d = d0 + l, and the wave walks the target columns j, so that at every step
//   * the target letter t[j] is wave-uniform (sixteen letters per load, handed to the scalar unit),
//   * lane l needs the query row i = j + d0 + l, i.e. the 64 lanes read 64 CONSECUTIVE entries of the query profile of letter t[j]:
//     one conflict-free LDS read, whose address is lane constant + scalar (one v_add),
//   * run and best never leave the lane - no cross-lane move in the loop, no carry between column tiles, and the diagonal of the maximum is
//     known for free (it is the lane); a wave reduction per pair picks (max score, smallest diagonal).
// Two queries share a workgroup's profile: an entry is { S3[qA[i]][c] + biasA[i], S3[qB[i]][c] + biasB[i] } as packed int16, so a step is
// v_add_u32 (address) + ds_read_b32 + v_pk_add_i16 clamp + v_pk_max_i16 (with 0) + v_pk_max_i16 (best): 4 VALU operations per 2 cells, against
// 5 packed operations + the DPP moves of the gapped recurrence.  Rows outside a query (before its start, behind its end, the shorter query of a
// pair) read 0 from the profile's padding: run keeps its value, best cannot grow.  The add saturates at 32767; a run that gets there has long
// passed the cap of 255, so the capped result is exact for every length.
//
// Length classes: the queries of a batch are sorted by length and paired with their neighbour, a pair belongs to the smallest class whose row count
// holds its longer query: 128 / 320 / 640 rows in LDS (21 letters x (rows + 128) x 4 B: 21 / 37 / 63 KiB; a CU's 32 wave slots hold 4 workgroups of
// 512 threads, so the first two classes run 4 per CU and the 640-row class, bound by the 160 KiB of LDS, 2), and beyond that the same kernel reads a profile built in device memory (any length up to 65,535).
#include "uc_engine.h"

namespace uc {

typedef short pk16 __attribute__((ext_vector_type(2)));

constexpr int UA_THREADS = 512, UA_WAVES = UA_THREADS / 64;
constexpr int UA_PAD = 64;                                         // zero entries in front of and behind a letter's profile row
constexpr int UA_CLASS_ROWS[3] = {128, 320, 640};                  // LDS classes; longer queries: profile in device memory
constexpr uint64_t UA_LONG_PROFILE_BYTES = 64ull << 20;            // device-memory profiles of one launch of the long class (at least one pair)

struct UaPair { uint32_t qa, qb; };                                // qb = UINT32_MAX: an odd query out

// profile of the pair for all 21 target letters: dst[c * rs + UA_PAD + i], i in [0, lmax); zero elsewhere
__device__ __forceinline__ void ua_build_profile(uint32_t *dst, int rs, const DeviceDb &db, uint32_t qa, uint32_t qb, int la, int lb) {
    const uint8_t *a3 = db.s3 + db.off[qa], *b3 = lb ? db.s3 + db.off[qb] : nullptr;
    const int8_t *ba = db.bias ? db.bias + db.off[qa] : nullptr, *bb = (db.bias && lb) ? db.bias + db.off[qb] : nullptr;
    for (int x = threadIdx.x; x < rs; x += blockDim.x) {
        const int i = x - UA_PAD;
        const bool ina = i >= 0 && i < la, inb = i >= 0 && i < lb;
        const int ra = ina ? a3[i] * 21 : 0, rb = inb ? b3[i] * 21 : 0;
        const int xa = ina && ba ? ba[i] : 0, xb = inb && bb ? bb[i] : 0;
        for (int c = 0; c < 21; c++) {
            const int lo = ina ? db.S3[ra + c] + xa : 0, hi = inb ? db.S3[rb + c] + xb : 0;
            dst[c * rs + x] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
        }
    }
}

__global__ void __launch_bounds__(256) ua_profile_kernel(const DeviceDb db, const UaPair *pairs, const uint64_t *poff, uint32_t *prof) {
    const UaPair p = pairs[blockIdx.x];
    const int la = (int)db.len[p.qa], lb = p.qb != UINT32_MAX ? (int)db.len[p.qb] : 0;
    ua_build_profile(prof + poff[blockIdx.x], max(la, lb) + 2 * UA_PAD, db, p.qa, p.qb, la, lb);
}

// score[(q - q0) * nt + (t - t0)], diag[...] for the queries of `pairs` against the targets [t0, t0 + nt).  blockIdx.x = pair, blockIdx.y = target slice.
template <bool LDS_PROFILE>
__global__ void __launch_bounds__(UA_THREADS) ungapped_all_kernel(const DeviceDb db, const UaPair *pairs, const uint64_t *poff, const uint32_t *gprof,
                                                                  uint32_t q0, uint32_t t0, uint32_t nt, uint8_t *score, int32_t *diag) {
    extern __shared__ uint32_t ua_lds[];
    const UaPair p = pairs[blockIdx.x];
    const int la = (int)db.len[p.qa], lb = p.qb != UINT32_MAX ? (int)db.len[p.qb] : 0;
    const int lmax = max(la, lb), rs = lmax + 2 * UA_PAD;
    const char *gp = nullptr;
    if constexpr (LDS_PROFILE) {
        ua_build_profile(ua_lds, rs, db, p.qa, p.qb, la, lb);
        __syncthreads();
    } else gp = (const char *)(gprof + poff[blockIdx.x]);
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const pk16 zero = {0, 0};
    for (uint32_t tt = blockIdx.y * UA_WAVES + wave; tt < nt; tt += gridDim.y * UA_WAVES) {
        const uint32_t t = t0 + tt;
        const int lt = (int)db.len[t];
        const uint8_t *t3 = db.s3 + db.off[t];
        const int dmin = -(lt - 1), ndiag = lmax + lt - 1;
        // best (capped score << 18 | 0x3ffff - (d - dmin)) of this lane's diagonals; the seed is score 0 on the first diagonal, so that a pair
        // whose diagonal loop does not run at all (an empty sequence) can never read as a score
        int ka = 0x3ffff, kb = 0x3ffff;
        for (int d0 = dmin; d0 < dmin + ndiag; d0 += 64) {
            // columns at which one lane at least is inside the rows [0, lmax): every read stays inside [1, rs - 2] of the letter's row
            const int jlo = max(0, -d0 - 63), jhi = min(lt - 1, lmax - 1 - d0);
            const int lo = 4 * (UA_PAD + d0 + lane);                // byte offset of this lane's row at column 0: lane constant + scalar per step
            pk16 run = zero, best = zero;
            auto step = [&](uint32_t c, int j) {
                const int so = 4 * ((int)min(c, 20u) * rs + j);
                pk16 s;
                if constexpr (LDS_PROFILE) s = *(const pk16 *)((const char *)ua_lds + (lo + so));
                else s = *(const pk16 *)(gp + (lo + so));
                run = __builtin_elementwise_max(__builtin_elementwise_add_sat(run, s), zero);
                best = __builtin_elementwise_max(best, run);
            };
            // the letters are wave-uniform: one vector load per 16 (4) columns, moved to the scalar unit, so that letter * rs + j is scalar arithmetic
            auto step4 = [&](uint32_t wv, int j) {
                const uint32_t w = __builtin_amdgcn_readfirstlane(wv);
                step(w & 0xffu, j); step((w >> 8) & 0xffu, j + 1); step((w >> 16) & 0xffu, j + 2); step(w >> 24, j + 3);
            };
            int j = jlo;
            for (; j <= jhi && (j & 3); j++) step(__builtin_amdgcn_readfirstlane((uint32_t)t3[j]), j);
            for (; j + 15 <= jhi; j += 16) {                       // (sequences start 16-byte aligned: j is a multiple of 4 here)
                uint32_t w[4];
                __builtin_memcpy(w, t3 + j, 16);
                step4(w[0], j); step4(w[1], j + 4); step4(w[2], j + 8); step4(w[3], j + 12);
            }
            for (; j + 3 <= jhi; j += 4) {
                uint32_t w;
                __builtin_memcpy(&w, t3 + j, 4);
                step4(w, j);
            }
            for (; j <= jhi; j++) step(__builtin_amdgcn_readfirstlane((uint32_t)t3[j]), j);
            const int back = 0x3ffff - (d0 - dmin + lane);
            ka = max(ka, (min((int)best.x, 255) << 18) | back);
            kb = max(kb, (min((int)best.y, 255) << 18) | back);
        }
        for (int o = 32; o > 0; o >>= 1) { ka = max(ka, __shfl_xor(ka, o, 64)); kb = max(kb, __shfl_xor(kb, o, 64)); }
        if (lane == 0) {      // a pair with an empty sequence has no cell and no diagonal: score 0, diag 0 (and it is never a candidate, ua_candidates_kernel)
            const size_t ia = (size_t)(p.qa - q0) * nt + tt;
            const bool ea = la == 0 || lt == 0, eb = lb == 0 || lt == 0;
            score[ia] = ea ? 0 : (uint8_t)(ka >> 18);
            diag[ia] = ea ? 0 : dmin + (0x3ffff - (ka & 0x3ffff));
            if (p.qb != UINT32_MAX) {
                const size_t ib = (size_t)(p.qb - q0) * nt + tt;
                score[ib] = eb ? 0 : (uint8_t)(kb >> 18);
                diag[ib] = eb ? 0 : dmin + (0x3ffff - (kb & 0x3ffff));
            }
        }
    }
}

// the tile's pairs with score >= min_score as candidate records (any order: the E4 selection sorts them)
__global__ void __launch_bounds__(256) ua_candidates_kernel(const uint8_t *score, const int32_t *diag, const uint32_t *len, uint32_t nq, uint32_t nt, uint32_t q0, uint32_t t0,
                                                            int min_score, uint32_t *cq, uint32_t *ct, int32_t *cs, int32_t *cd, unsigned long long *cursor) {
    const uint64_t n = (uint64_t)nq * nt;
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < n; i0 += (uint64_t)gridDim.x * 256) {
        const uint64_t i = i0 + threadIdx.x;
        const int s = i < n ? score[i] : -1;
        // an empty sequence is in no hit list, whatever the threshold: the gapped stage never sees a pair without cells
        const bool keep = s >= min_score && len[q0 + (uint32_t)(i / nt)] != 0 && len[t0 + (uint32_t)(i % nt)] != 0;
        const unsigned long long m = __ballot(keep);
        if (!m) continue;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        if (keep) {
            const uint64_t w = base + __popcll(m & ((1ull << lane) - 1));
            cq[w] = q0 + (uint32_t)(i / nt); ct[w] = t0 + (uint32_t)(i % nt); cs[w] = s; cd[w] = diag[i];
        }
    }
}

void ungapped_all_plan(uint64_t budget_bytes, uint32_t nq, uint32_t nt, uint32_t *qb, uint32_t *tc) {
    const uint64_t pairs = std::max<uint64_t>(1, budget_bytes / UNGAPPED_ALL_PAIR_BYTES);
    uint64_t r = 1;
    while ((r + 1) * (r + 1) <= pairs) r++;
    const uint32_t b = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)nq, 2048, r}));
    *qb = b;
    *tc = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nt, pairs / b));
}

static PerDeviceOnce ua_attr_once;

void ungapped_all_tile(Engine &E, UngappedAllWork &W, uint32_t q0, uint32_t q1, uint32_t t0, uint32_t t1) {
    const uint32_t nq = q1 - q0, nt = t1 - t0;
    if (!nq || !nt) return;
    W.score.reserve((size_t)nq * nt); W.diag.reserve((size_t)nq * nt);
    // pairs of neighbours in length order, grouped by class
    std::vector<uint32_t> order(nq);
    for (uint32_t i = 0; i < nq; i++) order[i] = q0 + i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return E.h_len[a] < E.h_len[b]; });
    std::vector<UaPair> pairs;
    uint32_t cls_begin[5] = {0, 0, 0, 0, 0};      // pairs [cls_begin[c], cls_begin[c + 1]) belong to class c (3 = long); lengths ascend, so classes do
    for (uint32_t i = 0; i < nq; i += 2) {
        const uint32_t qa = order[i], qb = i + 1 < nq ? order[i + 1] : UINT32_MAX;
        const uint32_t lmax = qb != UINT32_MAX ? E.h_len[qb] : E.h_len[qa];
        int c = 0;
        while (c < 3 && lmax > (uint32_t)UA_CLASS_ROWS[c]) c++;
        pairs.push_back({qa, qb});
        cls_begin[c + 1]++;
    }
    for (int c = 0; c < 4; c++) cls_begin[c + 1] += cls_begin[c];
    W.pairs.reserve(pairs.size() * 2);
    UC_HIP(hipMemcpyAsync(W.pairs.p, pairs.data(), pairs.size() * sizeof(UaPair), hipMemcpyHostToDevice, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    const UaPair *dp = (const UaPair *)W.pairs.p;
    ua_attr_once([] {
        UC_HIP(hipFuncSetAttribute((const void *)ungapped_all_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 21 * (UA_CLASS_ROWS[2] + 2 * UA_PAD) * 4));
    });
    auto grid_y = [&](uint32_t np) { return std::max<uint32_t>(1, std::min<uint32_t>((nt + 8 * UA_WAVES - 1) / (8 * UA_WAVES), (4096 + np - 1) / np)); };
    for (int c = 0; c < 3; c++) {
        const uint32_t np = cls_begin[c + 1] - cls_begin[c];
        if (!np) continue;
        const size_t lds = (size_t)21 * (UA_CLASS_ROWS[c] + 2 * UA_PAD) * 4;
        hipLaunchKernelGGL(ungapped_all_kernel<true>, dim3(np, grid_y(np)), dim3(UA_THREADS), lds, E.stream, E.ddb, dp + cls_begin[c], nullptr, nullptr,
                           q0, t0, nt, W.score.p, W.diag.p);
    }
    // long class: as many pairs per launch as UA_LONG_PROFILE_BYTES of profiles hold
    for (uint32_t a = cls_begin[3]; a < (uint32_t)pairs.size();) {
        std::vector<uint64_t> off;
        uint64_t words = 0;
        uint32_t b = a;
        while (b < pairs.size()) {
            const uint32_t lmax = pairs[b].qb != UINT32_MAX ? E.h_len[pairs[b].qb] : E.h_len[pairs[b].qa];
            const uint64_t w = 21ull * (lmax + 2 * UA_PAD);
            if (b > a && (words + w) * 4 > UA_LONG_PROFILE_BYTES) break;
            off.push_back(words);
            words += w;
            b++;
        }
        W.prof.reserve(words); W.prof_off.reserve(off.size());
        UC_HIP(hipMemcpyAsync(W.prof_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, E.stream));
        UC_HIP(hipStreamSynchronize(E.stream));
        const uint32_t np = b - a;
        hipLaunchKernelGGL(ua_profile_kernel, dim3(np), dim3(256), 0, E.stream, E.ddb, dp + a, W.prof_off.p, W.prof.p);
        hipLaunchKernelGGL(ungapped_all_kernel<false>, dim3(np, grid_y(np)), dim3(UA_THREADS), 0, E.stream, E.ddb, dp + a, W.prof_off.p, W.prof.p,
                           q0, t0, nt, W.score.p, W.diag.p);
        UC_HIP(hipStreamSynchronize(E.stream));      // the profile buffer is reused by the next launch
        a = b;
    }
    UC_HIP(hipGetLastError());
}

uint64_t ungapped_all_candidates(Engine &E, const UngappedAllWork &W, uint32_t q0, uint32_t nq, uint32_t t0, uint32_t nt, int min_score,
                                 uint32_t *cq, uint32_t *ct, int32_t *cs, int32_t *cd, unsigned long long *cursor) {
    UC_HIP(hipMemsetAsync(cursor, 0, 8, E.stream));
    hipLaunchKernelGGL(ua_candidates_kernel, grid_for((uint64_t)nq * nt), dim3(256), 0, E.stream, W.score.p, W.diag.p, E.ddb.len, nq, nt, q0, t0, min_score, cq, ct, cs, cd, cursor);
    unsigned long long n = 0;
    UC_HIP(hipMemcpyAsync(&n, cursor, 8, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    UC_HIP(hipGetLastError());
    return n;
}

// kernel-level entry: dense [nq][nt] scores and diagonals of queries [q0, q1) x targets [t0, t1), tile by tile under `tile_bytes` (0: the default budget)
void Engine::ungapped_all(uint32_t q0, uint32_t q1, uint32_t t0, uint32_t t1, uint64_t tile_bytes, int32_t *score_out, int32_t *diag_out) {
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    if (q0 > q1 || q1 > hdb.n || t0 > t1 || t1 > hdb.n) fail(UC_ERR_ARGS, "ungapped_all: bad query or target range");
    UC_HIP(hipSetDevice(device));
    const uint32_t nq = q1 - q0, nt = t1 - t0;
    if (!nq || !nt) return;
    uint32_t QB, TC;
    ungapped_all_plan(tile_bytes ? std::min(tile_bytes, UNGAPPED_ALL_TILE_BYTES) : UNGAPPED_ALL_TILE_BYTES, nq, nt, &QB, &TC);      // (a caller's budget can only shrink the tiles)
    UngappedAllWork W;
    std::vector<uint8_t> hs;
    std::vector<int32_t> hd;
    for (uint32_t qa = q0; qa < q1; qa += std::min(QB, q1 - qa))
        for (uint32_t ta = t0; ta < t1; ta += std::min(TC, t1 - ta)) {
            const uint32_t bq = std::min(QB, q1 - qa), bt = std::min(TC, t1 - ta), qe = qa + bq, te = ta + bt;
            ungapped_all_tile(*this, W, qa, qe, ta, te);
            hs.resize((size_t)bq * bt); hd.resize((size_t)bq * bt);
            UC_HIP(hipMemcpyAsync(hs.data(), W.score.p, hs.size(), hipMemcpyDeviceToHost, stream));
            UC_HIP(hipMemcpyAsync(hd.data(), W.diag.p, hd.size() * 4, hipMemcpyDeviceToHost, stream));
            UC_HIP(hipStreamSynchronize(stream));
            for (uint32_t i = 0; i < bq; i++)
                for (uint32_t k = 0; k < bt; k++) {
                    const size_t o = (size_t)(qa - q0 + i) * nt + (ta - t0 + k);
                    score_out[o] = hs[(size_t)i * bt + k];
                    diag_out[o] = hd[(size_t)i * bt + k];
                }
        }
}

}  // namespace uc
