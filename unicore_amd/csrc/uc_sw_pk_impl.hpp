// uc_sw_pk_impl.hpp — packed 16-bit variant of the gapped DP kernel (stage E5; see uc_sw_impl.hpp for the
// systolic-group design it shares).  The int32 kernel is integer-VALU-bound (every int32 VALU instruction
// occupies its SIMD for 4 cycles, profiles/round1/r1b_pmc_sw.txt), so the only lever left is instructions per cell:
// here every DP register holds TWO alignments of the same query (target A in the low, target B in the high
// 16 bits) and the recurrence runs on packed 16-bit VALU instructions, 8 per row and step (4 per cell) + 1 for the column and row maxima.
//
//  * biased domain (every MODE but 7): registers hold H' = H + 128 and E' = E + 128 in either half; F' = F + 128 too, but floored at a true -128 only.
//      x' = diag' + ub - 128   ONE plain 32-bit v_add3_u32 on the packed register, ub = s + 128 the profile byte sum and 0xFF7FFF80 (= -0x00800080) the
//                              third addend.  Per half diag' >= 128 and 0 <= ub <= 255, so the two-operand sum carries out of no half and the subtraction
//                              borrows from none.  (Written per half the constant would be 0xFF80FF80 - and wrong by one in the high half: the low half's sum
//                              with 0xFF80 ALWAYS carries.)  x' is not floored: it stands for Hdiag + s >= -128.
//      h'  = max3(x', e', f')  one v_pk_maximum3_f16 (see SW_PK_OVF).  e' >= 128 always, which is H's floor at a true 0.
//      E'' = max3(e' - ext, h' - open, 128)   saturating subtracts; the third operand floors E at a true 0, exactly what the saturating subtract does in
//                              the unbiased domain.  f'' = max(f' - ext, h' - open) needs no floor: a negative F never wins against e'.
//    That is perm + add3 + max3 + 3 subtracts + max3 + max = 8, where the unbiased domain needs 9 (x = sat_sub(sat_add(Hdiag, ub), 128) is two).  H and
//    E have the unbiased domain's value in every cell (tests/test_sw_bias_model.py: both recurrences cell by cell, the packed sums as 32-bit integers).
//    Resets: H, E, Hlast, prevHup, best, rowbest = 0x00800080; f enters lane 0 as 0; the diagonal that lane 0 receives (0 from the DPP shift) is raised
//    to the bias by one v_pk_max_u16 per step.  The three constants are SGPR operands of their instructions (pk_max3_s, pk_max_s, add3_s): no class
//    holds a wave per SIMD less than before (profiles/biased_domain/kernel_resources.txt).  Out of the kernel go best - 128 and the unbiased known score.
//  * overflow in the biased domain.  SW_PK_OVF stays 0x7C00 - 256 on the REPORTED (unbiased) score.  A reported score below it means every
//    h' stayed below 0x7C00 - 128: only patterns the f16 maximum orders like integers took part, the result is exact.  A true score of 0x7C00 - 128 or more
//    makes some h' >= 0x7C00, which every later max3 keeps (colmax) and the integer maximum `best` records: reported >= 0x7C00 - 128 > SW_PK_OVF.  So the
//    flagged pairs are exactly those of the unbiased domain.  The add no longer saturates, yet a half never carries into its neighbour - which belongs
//    to ANOTHER pair, whose result must stay exact: a stored value never exceeds 0x7FFF, because max3 returns one of its inputs or, if an input is a NaN
//    pattern (0x7C01 .. 0x7FFF), a NaN with a clear sign bit, and the subtracts and the integer max only lower a value or pick one; so x' <= 0x7FFF + 127.
//    An x' of 0x8000 .. 0x807E reads as a negative f16 and loses against e' >= 0x0080.  Both properties are checked exhaustively on the device by
//    tools/ubench/pk_max3_f16.hip (check_biased); v_add3_u32 and the SGPR forms issue at the rate of the instructions they replace (valu_rate.hip).
//  * MODE 7 keeps the unsigned floored domain (it stores H mod 256 for the walk): H >= 0, E/F/T floored at 0 by saturating subtraction (exact for
//    local alignment); x = sat_sub(sat_add(Hdiag, s + 128), 128) = max(Hdiag + s, 0); H = max3(x, e, f).
//  * profile bytes are (S3+64) and (SA+64) so the packed byte sum is s+128 (PAD = 0 => s = -128); one
//    v_perm_b32 per row interleaves byte r of target A's and target B's word into two zero-extended u16.
//  * first column of the maximum (MODE 0 / 2): ONE packed register age2 holds, per half, the steps since this lane's column maximum last exceeded its
//    running best.  Per step d = sat_sub(colmax, best) is non-zero exactly where the maximum rose (strictly: the FIRST column), nm = sat_sub(1, d) is
//    1 where it did not, and age2 = age2 * nm + nm (v_pk_mad_u16, mod 2^16, the rate of v_pk_sub_u16: valu_rate.hip) counts on or starts again at 0: three
//    packed instructions where two int32 column registers took an unpacking compare and a select each (-2 per step, one register less).  finish_slot
//    rebuilds the column as (nst - 1 - g) - age mod 2^16: exact, a column is below 65,535, even where nst or the age wrapped
//    (tests/test_sw_firstcol_model.py).  Integer operations only: a NaN pattern in colmax needs no special case.
//  * target letters, G < 64, every MODE but 7: one 32-bit load per target and 2-step trip brings the letters of two columns from the interleaved stream
//    a.db.lt (see LT2 in the kernel); one v_perm_b32 per step packs A's and B's half into c1.  -3 VALU and -1 VMEM instruction per step against one
//    16-bit load per target and step.  G = 64 reads its letters through the scalar cache, MODE 7 keeps the 16-bit loads.
//  * end tracking: per lane the running maximum gives (score, first column) per half; per-row maxima
//    (rowbest) identify the row: if exactly one row of the alignment ever reaches the optimum it must be the
//    row of the first column too, so (qEnd, tEnd) is exact.  Otherwise — or if a value came within 256 of the
//    packed score range (0x7C00, see SW_PK_OVF) — the pair is flagged (qEnd = -2 / score >= SW_PK_OVF): overflows are
//    re-run by the int32 kernel at once, ambiguous end rows only if the pair passes the E-value gate, by the
//    known-score variant of this kernel (MODE 4 / 6).
//  * slot streaming: a "slot" is two consecutive pairs of the task (A, B).  Every lane group pulls its next
//    slot from an LDS counter as soon as it has finished the previous one, so the groups of a wave do NOT
//    run in lockstep over the longest of their targets (hit lists mix family members with unrelated hits of
//    very different lengths; lockstep cost ~40 % of the issued instructions, profiles/round1/r1e).
#pragma once
#include <hip/hip_runtime.h>

#include "uc_device.h"
#include "uc_sw_impl.hpp"

namespace uc {

// H = max(x, e, f) is ONE instruction: v_pk_maximum3_f16 orders non-negative 16-bit integers below 0x7C00 (the f16
// infinity pattern) exactly like an unsigned max, denormal range included, at full rate, and returns >= 0x7C00 as
// soon as an operand is >= 0x7C00 (tools/ubench/pk_max3_f16.hip: exhaustive check on gfx950) - so the packed score
// range ends at 0x7C00 and an overflow is never lost (best/colmax are integer maxima, the flag is sticky).
constexpr int SW_PK_OVF = 0x7C00 - 256;   // scores at or above this are recomputed in int32

typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(4)));   // dword-aligned wide stores (MODE 7)
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef const uint32_t __attribute__((address_space(4))) *sw_cu32p;         // constant address space: uniform loads become s_load_dword
__device__ __forceinline__ u16x2_t pk_v(uint32_t x) { return __builtin_bit_cast(u16x2_t, x); }
__device__ __forceinline__ uint32_t pk_u(u16x2_t v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ uint32_t pk_add_sat(uint32_t a, uint32_t b) { return pk_u(__builtin_elementwise_add_sat(pk_v(a), pk_v(b))); }
__device__ __forceinline__ uint32_t pk_sub_sat(uint32_t a, uint32_t b) { return pk_u(__builtin_elementwise_sub_sat(pk_v(a), pk_v(b))); }
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) { return pk_u(__builtin_elementwise_max(pk_v(a), pk_v(b))); }
// inline asm: the compiler canonicalises min(x, 1) into compare + select per half (13 instructions instead of 1)
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_max3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// The constants of the biased domain are uniform: they reach their instruction as its one SGPR operand and cost no vector register.
__device__ __forceinline__ uint32_t pk_max3_s(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}
__device__ __forceinline__ uint32_t pk_max_s(uint32_t a, uint32_t c) {
    uint32_t r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "s"(c));
    return r;
}
__device__ __forceinline__ uint32_t add3_s(uint32_t a, uint32_t b, uint32_t c) {   // a plain 32-bit sum of three
    uint32_t r;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}
// per half a * b + c mod 2^16 (the first-column age of MODE 0: do_step)
__device__ __forceinline__ uint32_t pk_mad(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
constexpr uint32_t SW_PK_BIAS = 128u * 0x10001u;       // H' = H + 128, E' = E + 128 in either half (every MODE but 7)
constexpr uint32_t SW_PK_UNBIAS = 0u - SW_PK_BIAS;     // -128 in either half as ONE 32-bit addend: 0xFF7FFF80 (not 0xFF80FF80: see the header comment)
static_assert(SW_PK_UNBIAS == 0xFF7FFF80u, "the packed -128");

// K > 1: slots of the K tasks one workgroup serves (K * tcap / 2 at most: the launcher checks) and how a table entry names one: task << 6 | slot
constexpr int SW_MQ_SLOTS = 128;

template <int G, int R, int MODE, int NW, int K = 1>
__global__ void __launch_bounds__(NW * 64) sw_pk_kernel(const SwArgs a) {
    // K = tasks per workgroup.  K = 1: one task, its slots in list order.  K > 1 (G < 64, not MODE 7): workgroup b serves the tasks [K b, K b + K) of the
    // launch (the last one fewer), i.e. K neighbours of the plan's LPT order: one profile per task in LDS, and the lane groups pull the slots of ALL of them
    // from one table sorted by step count, longest first.  With one short list per workgroup (configs[1]: 8 slots on 8 lane groups in the reversed-query and
    // start passes) every wave issues for as long as its longest slot runs; K lists merged by length give every group several slots of similar length to even
    // that out (tools/slot_balance.py, profiles/multi_query_tasks).  Pair order, results and counters are those of K = 1.
    // MODE 4 / 6 = MODE 0 / 2 with the optimum score of every pair KNOWN (a.pscore).  MODE 4 is the exact re-run of the
    // pairs whose end row was ambiguous; MODE 6 is THE start pass of the packed path (its optimum is the forward score).
    // No per-row maxima: the first step at which a lane's column maximum equals the known score is its first optimal
    // column, and only at such steps (a rare, wave-level branch) the lane looks at its rows: first optimal row, and
    // whether a single row holds all optimal cells (the condition under which a mutual hit may share the result).
    // MODE 7 = traceback bytes: the forward DP on the box [qs..qe] x [ts..te] of an accepted pair; instead of tracking an
    // end position every cell of the diagonal band the traceback can reach (tb_band_of, uc_device.h; r05) stores ONE byte, H mod 256,
    // into a per-pair matrix in HBM, laid out by anti-diagonal step so that the lanes inside the band store NL*RB contiguous bytes per step.  No decision is computed here (r04: six compare bits per
    // cell had cost 16 of the pass's 27 VALU instructions per row and step; a byte of H costs the byte shuffle only).  A
    // second kernel (tb_walk_kernel, uc_sw_plan.hip) walks every pair's matrix from the end cell, whose H it knows (the
    // score): neighbouring cells differ by less than 128, so every H it needs is exact again, and every decision of the
    // traceback (diagonal / F / E, gap opened or extended) is a comparison of H values: alignment length, identities, gaps.
    constexpr bool TBB = MODE == 7;
    constexpr uint32_t HB = TBB ? 0u : SW_PK_BIAS;   // what a true 0 of H and E looks like in a register
    constexpr bool KNOWN = MODE == 4 || MODE == 6;
    constexpr int BASE = KNOWN ? MODE - 4 : (TBB ? 0 : MODE);
    constexpr bool TRACK = BASE != 1 && !TBB, MASK = BASE == 2 || TBB, REVQ = BASE != 0, REVT = BASE == 2;
    constexpr int RW = (R + 3) / 4, BW = RW | 1, RSW = G * BW, NT = NW * 64;   // R % 4 == 2: the last profile dword is half used
    static_assert(R % 2 == 0 && R <= 32, "R must be even, <= 32");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    static_assert(K == 1 || (K <= 4 && G < 64 && !TBB), "several tasks per workgroup: G < 64, not MODE 7");
    constexpr int PB = 2 * SW_NLET * RSW;           // dwords of one task's profile
    uint32_t *P3 = lds, *PA = lds + SW_NLET * RSW;
    uint32_t *slot_ctr = lds + K * PB;              // work counter of the workgroup (one dword behind the profiles)
    // K > 1, behind the counter: (begin, count, query length, [task 0: slots of all tasks]) per task; the step count of every slot (<< 8 | its name); the slot table
    [[maybe_unused]] uint32_t *tinfo = slot_ctr + 4, *sstep = tinfo + 4 * K;
    [[maybe_unused]] uint8_t *stab = (uint8_t *)(sstep + SW_MQ_SLOTS);

    const SwTask task = a.tasks[K * blockIdx.x];    // K > 1: the first of the workgroup's tasks
    const int tid = threadIdx.x, lane = tid & 63;
    const int g = lane % G;
    const uint32_t qoff = a.db.off[task.q];
    const int lq = (int)a.db.len[task.q];
    const uint32_t open2 = (uint32_t)a.open * 0x10001u, ext2 = (uint32_t)a.ext * 0x10001u, bias2 = 128u * 0x10001u;
    const uint32_t nslots = (task.count + 1) >> 1;

    // ---- query profile in LDS: bytes S3+64 and SA+64 (sum = s+128), PAD letters / rows = 0 ----
    // (r06, measured and not kept: the two 21 x 21 matrices and the query letters staged in LDS first, the entries assembled from LDS bytes instead of eight
    // dependent global round trips each - no change in any pass, the sparse ones included (mode 4 at configs[1]: 23.1 ms either way): the build is not
    // what a task waits for.  profiles/r06/sparse_passes.txt)
    for (int idx = tid; idx < SW_NLET * G * RW; idx += NT) {
        const int c = idx / (G * RW), rem = idx % (G * RW), gg = rem / RW, k = rem % RW;
        uint32_t w3 = 0, wa = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int row = gg * R + 4 * k + b;
            if (row < lq && c < 21 && 4 * k + b < R) {
                const int qi = REVQ ? lq - 1 - row : row;
                const int q3 = a.db.s3[qoff + qi], qa = a.db.sa[qoff + qi];
                w3 |= (uint32_t)(a.db.S3[q3 * 21 + c] + 64) << (8 * b);
                wa |= (uint32_t)(a.db.SA[qa * 21 + c] + 64) << (8 * b);
            }
        }
        P3[c * RSW + gg * BW + k] = w3;
        PA[c * RSW + gg * BW + k] = wa;
    }
    if constexpr (K > 1) {
        // the other tasks' profiles (the loop above, one more index); every slot of the K tasks with its step count (entries in (task, slot) order); then
        // the slots ranked by (step count descending, task, slot) into the table start_slot reads.  Both barriers stand before the slot loop: none inside it.
        const uint32_t task0 = (uint32_t)K * blockIdx.x, nk = min((uint32_t)K, a.n_tasks - task0);
        uint32_t base[K + 1];
        base[0] = 0; base[1] = nslots;
        if (tid == 0) { tinfo[0] = task.begin; tinfo[1] = task.count; tinfo[2] = (uint32_t)lq; }
#pragma unroll
        for (int t = 1; t < K; t++) {
            base[t + 1] = base[t];
            if ((uint32_t)t < nk) {
                const SwTask tk = a.tasks[task0 + t];
                const uint32_t qofft = a.db.off[tk.q];
                const int lqt = (int)a.db.len[tk.q];
                for (int idx = tid; idx < SW_NLET * G * RW; idx += NT) {
                    const int c = idx / (G * RW), rem = idx % (G * RW), gg = rem / RW, k = rem % RW;
                    uint32_t w3 = 0, wa = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int row = gg * R + 4 * k + b;
                        if (row < lqt && c < 21 && 4 * k + b < R) {
                            const int qi = REVQ ? lqt - 1 - row : row;
                            const int q3 = a.db.s3[qofft + qi], qa = a.db.sa[qofft + qi];
                            w3 |= (uint32_t)(a.db.S3[q3 * 21 + c] + 64) << (8 * b);
                            wa |= (uint32_t)(a.db.SA[qa * 21 + c] + 64) << (8 * b);
                        }
                    }
                    P3[t * PB + c * RSW + gg * BW + k] = w3;
                    PA[t * PB + c * RSW + gg * BW + k] = wa;
                }
                base[t + 1] += (tk.count + 1) >> 1;
                if (tid == 0) { tinfo[4 * t] = tk.begin; tinfo[4 * t + 1] = tk.count; tinfo[4 * t + 2] = (uint32_t)lqt; }
            }
        }
        const uint32_t mq_slots = min(base[K], (uint32_t)SW_MQ_SLOTS);   // slots of all tasks of the workgroup
        if (tid == 0) tinfo[3] = mq_slots;
        for (uint32_t e = tid; e < mq_slots; e += NT) {
            uint32_t t = 0;
#pragma unroll
            for (int j = 1; j < K; j++) t += e >= base[j] ? 1u : 0u;
            uint32_t eb = 0;
#pragma unroll
            for (int j = 1; j < K; j++) eb = t == (uint32_t)j ? base[j] : eb;
            const SwTask tk = a.tasks[task0 + t];
            const uint32_t i = e - eb, pA = tk.begin + 2 * i, pB = pA + (2 * i + 1 < tk.count ? 1u : 0u);
            const int la = REVT ? a.pte[pA] + 1 : (int)a.db.len[a.pt[pA]], lb = REVT ? a.pte[pB] + 1 : (int)a.db.len[a.pt[pB]];
            sstep[e] = ((uint32_t)((max(la, lb) + G) & ~1) << 8) | (t << 6) | i;
        }
    }
    if (tid == 0) *slot_ctr = 0;
    __syncthreads();
    if constexpr (K > 1) {
        const uint32_t mq_slots = tinfo[3];
        for (uint32_t e = tid; e < mq_slots; e += NT) {
            const uint32_t v = sstep[e], s = v >> 8;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < mq_slots; j++) {
                const uint32_t sj = sstep[j] >> 8;
                rank += (sj > s || (sj == s && j < e)) ? 1u : 0u;
            }
            stab[rank] = (uint8_t)(v & 0xffu);
        }
        __syncthreads();
    }

    // ---- per-group state (all group-uniform scalars live replicated in the group's lanes) ----
    uint32_t H[R], E[R], rowbest[(TRACK && !KNOWN) ? R : 1];   // E[r] holds the gap state ENTERING the next column (no separate H - open array)
    uint32_t mskA[MASK ? RW : 1], mskB[MASK ? RW : 1];
    uint32_t best = HB, Hlast = HB, prevHup = HB, fout = 0;
    // KNOWN: colA / colB hold the lane's whole first-answer state in one register, so that the second key below costs no occupancy step:
    // -1 = no optimal cell yet, else first optimal column << 6 | its first row (of this lane's R) << 1 | this lane saw the optimum in more than one of its rows
    int colA = -1, colB = -1;
    // MODE 0 / 2 keep the first column of the maximum on ONE packed register instead: per half the steps since this lane's column maximum last exceeded
    // its running best (mod 2^16); finish_slot turns it back into the column
    [[maybe_unused]] uint32_t age2 = 0;
    [[maybe_unused]] uint32_t knownA = 0, knownB = 0;
    // KNOWN: the other tie-break order over this lane's optimal cells, (first optimal row, then first column) = row << 16 | col: the answer of the
    // transposed DP, i.e. of the mirror (t,q) of a mutual hit.  Only touched inside the event branch.
    [[maybe_unused]] int key2A = 0x7fffffff, key2B = 0x7fffffff;
    uint32_t gA = 0, gB = 0, toffA = 0, toffB = 0;
    [[maybe_unused]] unsigned long long tbA = 0, tbB = 0;
    [[maybe_unused]] int tsaA = 0, tsbA = 0, tsaB = 0, tsbB = 0;        // MODE 7: the steps in which this lane is inside the pair's stored band
    [[maybe_unused]] uint32_t trowA = 0, trowB = 0, tslotA = 0, tslotB = 0;   // ... bytes per step of the pair's matrix, this lane's byte offset in a step
    int tlenA = 0, tlenB = 0, rowoffA = 0, rowoffB = 0;
    bool vB = false, active = false;
    int lst = 0, nst = 0;
    uint32_t c1 = 0, cin = 0;
    struct RawLetters { uint32_t a3, aa, b3, ba; } r2 = {0, 0, 0, 0};   // G < 64: a3 / b3 hold the whole 16-bit letter pair
    uint32_t nA3[RW], nAa[RW], nB3[RW], nBa[RW];
    // G < 64: both letters of a residue come from the interleaved stream a.db.lt (3Di | AA << 8, PAD pairs between the
    // sequences): MODE 7 one 16-bit load per target and step, the index clamped onto the PAD entry behind the
    // sequence, so neither a second byte load nor a "past the end" select is needed.  ltA / ltB point at element 0.
    [[maybe_unused]] const uint16_t *ltA = nullptr, *ltB = nullptr;
    // G < 64, every MODE but 7 (LT2): ONE 32-bit load per target and 2-step trip brings the letters of two columns.  A sequence starts at a multiple of 16
    // entries and at least 16 PAD entries follow it (Engine::plan_db_layout; 16 more stand in front of the first), so:
    //  * forward targets: word (c, c + 1), c even, is ltA[min(c, clA)], clA = (tlen + 1) & ~1: even, hence 4-byte aligned; the clamp lands on
    //    (last, PAD) or (PAD, PAD), never on the sequence behind.  The low half is the first column of the two.
    //  * REVT: column c is element tlen - 1 - c.  ltA points two entries in front of the sequence and the word is ltA[max(tlen - c, 0)]: (c + 1, c) in
    //    its (low, high) half, (PAD, PAD) from the entries in front once c >= tlen, never the sequence in front.  An odd tlen makes these words
    //    2-byte aligned only (one global_load_dword all the same).
    // wA / wB hold the word whose columns enter c1 in this trip; the ODD step issues the next one right after it took the second half, one step before
    // its first use - the distance the 16-bit loads had.
    constexpr bool LT2 = G != 64 && !TBB;
    constexpr uint32_t LT2_FIRST = REVT ? 0x07060302u : 0x05040100u, LT2_SECOND = REVT ? 0x05040100u : 0x07060302u;   // v_perm_b32: [A's half | B's half << 16]
    [[maybe_unused]] uint32_t wA = 0, wB = 0;
    [[maybe_unused]] int clA = 0, clB = 0;
    typedef uint32_t __attribute__((aligned(2))) lt2_word;
    auto issue_words = [&](int c) __attribute__((always_inline)) {
        const uint32_t ia = REVT ? (uint32_t)max(clA - c, 0) : (uint32_t)min(c, clA);
        const uint32_t ib = REVT ? (uint32_t)max(clB - c, 0) : (uint32_t)min(c, clB);
        if constexpr (REVT) { wA = *(const lt2_word *)(ltA + ia); wB = *(const lt2_word *)(ltB + ib); }
        else { wA = *(const uint32_t *)(ltA + ia); wB = *(const uint32_t *)(ltB + ib); }
    };

    // letters of both targets travel as one dword: [c3A | caA << 8 | c3B << 16 | caB << 24].  The loads are
    // branch-free (clamped index, every lane of the group reads the same address) and are only combined a full
    // step after they were issued, so no step waits on global-memory latency.
    auto issue_letters = [&](int st) -> RawLetters {
        RawLetters r;
        if constexpr (G == 64) {   // one group per wave: the slot state is wave-uniform, so the letters come through the scalar
                                   // cache (aligned dword + shift on the SALU) and cost no VALU issue slots at all
            const int ia = max(min(st, tlenA - 1), 0), ib = max(min(st, tlenB - 1), 0);
            const uint32_t pa = toffA + (uint32_t)(REVT ? max(tlenA - 1 - ia, 0) : ia);
            const uint32_t pb_ = toffB + (uint32_t)(REVT ? max(tlenB - 1 - ib, 0) : ib);
            auto ld = [&](const uint8_t *base, uint32_t p) -> uint32_t {
                const sw_cu32p w = (sw_cu32p)(uintptr_t)(base + (p & ~3u));
                return (*w >> (8u * (p & 3u))) & 0xffu;
            };
            r.a3 = ld(a.db.s3, pa); r.aa = ld(a.db.sa, pa); r.b3 = ld(a.db.s3, pb_); r.ba = ld(a.db.sa, pb_);
        } else {   // MODE 7 only (LT2 otherwise)
            const uint32_t ia = (uint32_t)min(st, tlenA), ib = (uint32_t)min(st, tlenB);
            r.a3 = ltA[ia]; r.b3 = ltB[ib];
            r.aa = 0; r.ba = 0;
        }
        return r;
    };
    auto pack_letters = [&](const RawLetters &r, int st) -> uint32_t {
        if constexpr (G == 64) {
            const uint32_t ca_ = st < tlenA ? (r.a3 | (r.aa << 8)) : SW_PADPACK;
            const uint32_t cb_ = st < tlenB ? (r.b3 | (r.ba << 8)) : SW_PADPACK;
            return ca_ | (cb_ << 16);
        } else if constexpr (TBB) {   // a box ends inside its sequence: the columns past it are PAD by selection
            return (st < tlenA ? r.a3 : SW_PADPACK) | ((st < tlenB ? r.b3 : SW_PADPACK) << 16);
        } else {
            return r.a3 | (r.b3 << 16);
        }
    };
    uint32_t off3 = (uint32_t)(g * BW) * 4u, offa = (uint32_t)(SW_NLET * RSW + g * BW) * 4u;   // K > 1: + the slot's task x profile bytes (start_slot)
    asm volatile("" : "+v"(off3), "+v"(offa));
    auto fetch_profile = [&]() __attribute__((always_inline)) {
        // byte offsets: letter * row-set stride + this lane's base in P3 / PA (two opaque registers, so that the PA base is
        // the addend of the multiply-add instead of a separate add per load)
        const char *l8 = (const char *)lds;
        const uint32_t *pA3 = (const uint32_t *)(l8 + (cin & 0xff) * (RSW * 4) + off3), *pAa = (const uint32_t *)(l8 + ((cin >> 8) & 0xff) * (RSW * 4) + offa);
        const uint32_t *pB3 = (const uint32_t *)(l8 + ((cin >> 16) & 0xff) * (RSW * 4) + off3), *pBa = (const uint32_t *)(l8 + (cin >> 24) * (RSW * 4) + offa);
#pragma unroll
        for (int k = 0; k < RW; k++) { nA3[k] = pA3[k]; nAa[k] = pAa[k]; nB3[k] = pB3[k]; nBa[k] = pBa[k]; }
    };

    // pull the next slot of the task for this group and reset the group's DP state (group-uniform control flow)
    auto start_slot = [&]() {
        uint32_t idx = 0;
        if (g == 0) idx = atomicAdd(slot_ctr, 1u);
        if constexpr (G == 64) idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);   // wave-uniform from here on (SGPRs)
        else idx = (uint32_t)__shfl((int)idx, lane - g, 64);
        if constexpr (K == 1) active = idx < nslots;
        else active = idx < tinfo[3];
        if (!active) return;
        [[maybe_unused]] uint32_t mq_begin = 0, mq_count = 0;
        [[maybe_unused]] int mq_lq = 0;
        if constexpr (K > 1) {   // the slot's own task: its pairs, its query length, its profile
            const uint32_t code = stab[idx], t = code >> 6;
            idx = code & 63u;
            mq_begin = tinfo[4 * t]; mq_count = tinfo[4 * t + 1]; mq_lq = (int)tinfo[4 * t + 2];
            off3 = (t * PB + (uint32_t)(g * BW)) * 4u;
            offa = off3 + (uint32_t)(SW_NLET * RSW) * 4u;
        }
        const uint32_t iA = 2 * idx, iB = iA + 1;
        vB = iB < (K == 1 ? task.count : mq_count);
        gA = (K == 1 ? task.begin : mq_begin) + iA;
        gB = (K == 1 ? task.begin : mq_begin) + (vB ? iB : iA);
        const uint32_t tA = a.pt[gA], tB = a.pt[gB];
        toffA = a.db.off[tA]; toffB = a.db.off[tB];
        tlenA = REVT ? a.pte[gA] + 1 : (int)a.db.len[tA];
        tlenB = vB ? (REVT ? a.pte[gB] + 1 : (int)a.db.len[tB]) : 0;
        if constexpr (TBB) {   // the box: target slice [ts, te], query rows [qs, qe]
            toffA += (uint32_t)a.pts[gA]; toffB += (uint32_t)a.pts[gB];
            tlenA = a.pte[gA] - a.pts[gA] + 1;
            tlenB = vB ? a.pte[gB] - a.pts[gB] + 1 : 0;
            tbA = a.tboff[gA]; tbB = a.tboff[gB];
            const int qsA = a.pqs[gA], qeA = a.pqe[gA], qsB = a.pqs[gB], qeB = a.pqe[gB];
            {   // the stored band of either pair (tb_band_of, uc_device.h)
                constexpr int RBc = 4 * RW;
                const TbBand bA = tb_band_of(qsA, qeA, tlenA, G, R, a.tb_band), bB = tb_band_of(qsB, qeB, vB ? tlenB : 1, G, R, a.tb_band);
                const bool fullA = bA.nl >= G, fullB = bB.nl >= G;
                tsaA = fullA ? 0 : g * (R + 1) - bA.dhi; tsbA = fullA ? 0x7fffffff : g * (R + 1) + R - 1 - bA.dlo;
                tsaB = fullB ? 0 : g * (R + 1) - bB.dhi; tsbB = fullB ? 0x7fffffff : g * (R + 1) + R - 1 - bB.dlo;
                trowA = (uint32_t)(bA.nl * RBc); trowB = (uint32_t)(bB.nl * RBc);
                tslotA = (uint32_t)((g % bA.nl) * RBc); tslotB = (uint32_t)((g % bB.nl) * RBc);
            }
#pragma unroll
            for (int k = 0; k < RW; k++) {
                uint32_t ma = 0, mb = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int row = g * R + 4 * k + b;
                    ma |= (row >= qsA && row <= qeA ? 0xFFu : 0u) << (8 * b);
                    mb |= (row >= qsB && row <= qeB ? 0xFFu : 0u) << (8 * b);
                }
                mskA[k] = ma; mskB[k] = mb;
            }
        } else if constexpr (MASK) {
            rowoffA = (K == 1 ? lq : mq_lq) - 1 - a.pqe[gA];
            rowoffB = (K == 1 ? lq : mq_lq) - 1 - a.pqe[gB];
#pragma unroll
            for (int k = 0; k < RW; k++) {
                uint32_t ma = 0, mb = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    ma |= (g * R + 4 * k + b >= rowoffA ? 0xFFu : 0u) << (8 * b);
                    mb |= (g * R + 4 * k + b >= rowoffB ? 0xFFu : 0u) << (8 * b);
                }
                mskA[k] = ma; mskB[k] = mb;
            }
        }
        if constexpr (LT2) {
            ltA = a.db.lt + toffA - (REVT ? 2 : 0);
            // no second pair (tlenB = 0): every word is the two PAD entries in front of A's first residue
            ltB = vB ? a.db.lt + toffB - (REVT ? 2 : 0) : a.db.lt + toffA - 2;
            clA = REVT ? tlenA : (tlenA + 1) & ~1;
            clB = REVT ? tlenB : (tlenB + 1) & ~1;
        } else if constexpr (G != 64) {
            ltA = a.db.lt + toffA;
            // no second pair: every index lands on a PAD entry (the one before A's first residue)
            ltB = vB ? a.db.lt + toffB : a.db.lt + toffA - 1;
        }
#pragma unroll
        for (int r = 0; r < R; r++) { H[r] = HB; E[r] = HB; }
        if constexpr (TRACK && !KNOWN) {
#pragma unroll
            for (int r = 0; r < R; r++) rowbest[r] = HB;
        }
        if constexpr (KNOWN) {   // compared with the biased column maximum: known + 128 (128 = no known score: the guard of the event test)
            knownA = (uint32_t)a.pscore[gA] + 128u;
            knownB = vB ? (uint32_t)a.pscore[gB] + 128u : 128u;
            key2A = 0x7fffffff; key2B = 0x7fffffff;
        }
        best = HB; colA = -1; colB = -1; age2 = 0; Hlast = HB; prevHup = HB; fout = 0;   // f enters as 0 = true -128: it never wins against e' >= 128
        lst = 0;
        nst = (max(tlenA, tlenB) + G) & ~1;      // Lt + G - 1 steps, rounded up to the 2-step loop trip
        if constexpr (LT2) {   // columns 0 and 1 from the first word, the word of columns 2 and 3 in flight
            issue_words(0);
            const uint32_t c0 = __builtin_amdgcn_perm(wB, wA, LT2_FIRST);
            c1 = __builtin_amdgcn_perm(wB, wA, LT2_SECOND);
            issue_words(2);
            cin = (uint32_t)shift_from_prev_lane<G>((int)(SW_PADPACK * 0x10001u), (int)c0, g);
            fetch_profile();
            return;
        }
        c1 = pack_letters(issue_letters(1), 1);
        r2 = issue_letters(2);
        if constexpr (G == 64) {   // keep the letter pipeline in SGPRs across the loop back edge
            c1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)c1);
            r2.a3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r2.a3); r2.aa = (uint32_t)__builtin_amdgcn_readfirstlane((int)r2.aa);
            r2.b3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)r2.b3); r2.ba = (uint32_t)__builtin_amdgcn_readfirstlane((int)r2.ba);
        }
        cin = (uint32_t)shift_from_prev_lane<G>((int)(SW_PADPACK * 0x10001u), (int)pack_letters(issue_letters(0), 0), g);
        fetch_profile();
    };

    // ODD = second step of the 2-step loop trip: the per-row maxima take this step's and the previous step's H in one max3
    auto do_step = [&](const int st, const bool ODD) __attribute__((always_inline)) {
        uint32_t sA[RW], sB[RW];
#pragma unroll
        for (int k = 0; k < RW; k++) {
            sA[k] = nA3[k] + nAa[k];
            sB[k] = nB3[k] + nBa[k];
            if constexpr (MASK) { sA[k] &= mskA[k]; sB[k] &= mskB[k]; }
        }
        cin = (uint32_t)shift_from_prev_lane<G>((int)cin, (int)c1, g);
        if constexpr (LT2) {   // column st + 2: the first half of the trip's word in the even step, the second in the odd one, which then issues the next word
            c1 = __builtin_amdgcn_perm(wB, wA, ODD ? LT2_SECOND : LT2_FIRST);
            if (ODD) issue_words(st + 3);
        } else {
            c1 = pack_letters(r2, st + 2);
            r2 = issue_letters(st + 3);
        }
        fetch_profile();
        const uint32_t Hup = (uint32_t)shift_from_prev_lane_zero<G>((int)Hlast, g);
        uint32_t f = (uint32_t)shift_from_prev_lane_zero<G>((int)fout, g);
        // lane g = 0 received 0 from the shift: its diagonal is the bias (a true 0); every other lane's value is >= the bias already.  Raised here, at its
        // use, and not on Hup: that keeps one register less alive across the row loop (profiles/biased_domain/README.md, 3)
        uint32_t diag = prevHup;
        if constexpr (!TBB) diag = pk_max_s(prevHup, HB);
        uint32_t colmax = 0;
        [[maybe_unused]] uint32_t code[TBB ? R : 1];
#pragma unroll
        for (int r = 0; r < R; r++) {
            // {byte r of A's word, 0, byte r of B's word, 0}
            const uint32_t ub = __builtin_amdgcn_perm(sB[r >> 2], sA[r >> 2], 0x0c000c00u | ((4u + (r & 3)) << 16) | (uint32_t)(r & 3));
            // biased: x' = diag' + ub - 128 per half in one 32-bit add; not floored (it stands for Hdiag + s >= -128), e' >= 128 is H's floor
            uint32_t x;
            if constexpr (TBB) x = pk_sub_sat(pk_add_sat(diag, ub), bias2);
            else x = add3_s(diag, ub, SW_PK_UNBIAS);
            const uint32_t e = E[r];                          // max(E - ext, H - open) of the previous column
            const uint32_t h = pk_max3(x, e, f);
            const uint32_t hprev = H[r];                      // this row one column earlier
            diag = hprev;
            H[r] = h;
            const uint32_t t = pk_sub_sat(h, open2);
            const uint32_t esub = pk_sub_sat(e, ext2), fsub = pk_sub_sat(f, ext2);
            if constexpr (TBB) code[r] = h;   // the cell's byte = H mod 256 of either half (packed into byte streams below)
            if constexpr (TBB) E[r] = pk_max(esub, t);
            else E[r] = pk_max3_s(esub, t, HB);           // the third operand floors E at a true 0, as the saturating subtract does in the unbiased domain
            f = pk_max(fsub, t);
            if constexpr (TRACK && !KNOWN) { if (ODD) rowbest[r] = pk_max3(rowbest[r], hprev, h); }
            if (r & 1) colmax = pk_max3(colmax, H[r - 1], h);   // two rows per instruction (R is even)
        }
        if constexpr (TBB) {   // bytes of 4 rows -> one dword per pair; step-major matrix: G*RB contiguous bytes per group and step
            uint32_t wa[RW], wb[RW];
#pragma unroll
            for (int k = 0; k < RW; k++) {
                const uint32_t c0 = code[4 * k], c1_ = 4 * k + 1 < R ? code[4 * k + 1] : 0u;
                const uint32_t c2 = 4 * k + 2 < R ? code[4 * k + 2] : 0u, c3 = 4 * k + 3 < R ? code[4 * k + 3] : 0u;
                const uint32_t p01 = __builtin_amdgcn_perm(c1_, c0, 0x06020400u);   // [A0, A1, B0, B1]
                const uint32_t p23 = __builtin_amdgcn_perm(c3, c2, 0x06020400u);    // [A2, A3, B2, B3]
                wa[k] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
                wb[k] = __builtin_amdgcn_perm(p23, p01, 0x07060302u);
            }
            // every lane writes its RB bytes with as few (dword-aligned) wide stores as possible: the lanes of a group cover
            // G*RB contiguous bytes, so the stores of a step fill whole lines; streaming (written once, read sparsely)
            // (a step's row holds the lanes inside the pair's band only: trow = NL * RB bytes, this lane at tslot)
            uint8_t *dA = a.tbm + tbA + (unsigned long long)st * trowA + tslotA;
            uint8_t *dB = a.tbm + tbB + (unsigned long long)st * trowB + tslotB;
            auto put = [&](uint8_t *d, const uint32_t *w) __attribute__((always_inline)) {
                int k = 0;
#pragma unroll
                for (; k + 4 <= RW; k += 4) {
                    u32x4_u v = {w[k], w[k + 1], w[k + 2], w[k + 3]};
                    *(u32x4_u *)(d + 4 * k) = v;
                }
#pragma unroll
                for (; k + 2 <= RW; k += 2) {
                    u32x2_u v = {w[k], w[k + 1]};
                    *(u32x2_u *)(d + 4 * k) = v;
                }
#pragma unroll
                for (; k < RW; k++) *(uint32_t *)(d + 4 * k) = w[k];
            };
            if (st >= tsaA && st <= tsbA) put(dA, wa);
            if (vB && st >= tsaB && st <= tsbB) put(dB, wb);
        }
        if constexpr (TRACK && !KNOWN) {
            // strictly above best = the FIRST column of the maximum: d != 0 there, nm = 1 - min(d, 1), age = improved ? 0 : age + 1 in one multiply-add.
            // Integer operations throughout: a NaN pattern in colmax (an overflowed pair, re-run anyway) is a large number like any other.
            const uint32_t d = pk_sub_sat(colmax, best);
            const uint32_t nm = pk_sub_sat(0x00010001u, d);
            age2 = pk_mad(age2, nm, nm);
        }
        if constexpr (KNOWN) {
            // every column of this lane that holds the optimum is an event (a handful per alignment: wave-level branch);
            // the first one gives (column, row); all of them together tell whether ONE row holds every optimal cell
            const bool evA = knownA != 128u && (colmax & 0xffffu) == knownA;
            const bool evB = knownB != 128u && (colmax >> 16) == knownB;
            if (__builtin_amdgcn_ballot_w64(evA || evB) != 0) {
                if (evA) {
                    int first = 0, cnt = 0;
#pragma unroll
                    for (int r = R - 1; r >= 0; r--) { const bool hit = (H[r] & 0xffffu) == knownA; first = hit ? r : first; cnt += hit ? 1 : 0; }
                    if (colA < 0) colA = ((st - g) << 6) | (first << 1);
                    if constexpr (MODE == 6) colA |= (cnt > 1 || first != ((colA >> 1) & 31)) ? 1 : 0;   // (only MODE 6 reports the one-row mark)
                    key2A = min(key2A, ((g * R + first) << 16) | (st - g));   // columns ascend: a smaller row wins, an equal row keeps the earlier column
                }
                if (evB) {
                    int first = 0, cnt = 0;
#pragma unroll
                    for (int r = R - 1; r >= 0; r--) { const bool hit = (H[r] >> 16) == knownB; first = hit ? r : first; cnt += hit ? 1 : 0; }
                    if (colB < 0) colB = ((st - g) << 6) | (first << 1);
                    if constexpr (MODE == 6) colB |= (cnt > 1 || first != ((colB >> 1) & 31)) ? 1 : 0;
                    key2B = min(key2B, ((g * R + first) << 16) | (st - g));
                }
            }
        }
        best = pk_max(best, colmax);
        Hlast = H[R - 1];
        fout = f;
        prevHup = Hup;
    };

    // per-half reduction over the G lanes: (score desc, col asc); then the row from rowbest; write results
    auto finish_slot = [&]() {
        if constexpr (TBB) return;
        if constexpr (KNOWN) {
            knownA -= 128u; knownB -= 128u;   // unbiased for the output, in place: start_slot sets both anew
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int st1 = half ? colB : colA, col = st1 >> 6, row = (st1 >> 1) & 31;
                int key = st1 < 0 ? 0x7fffffff : ((col << 11) | (g * R + row));      // (first optimal column, then first row)
                // lanes that saw the optimum, + G if one of them saw it in two rows: exactly 1 <=> one row holds every optimal cell
                int nrows = st1 < 0 ? 0 : 1 + ((st1 & 1) ? G : 0);
                int key2 = half ? key2B : key2A;                                      // (first optimal row, then first column)
#pragma unroll
                for (int m = 1; m < G; m <<= 1) {
                    key = min(key, __shfl_xor(key, m, 64));
                    nrows += __shfl_xor(nrows, m, 64);
                    key2 = min(key2, __shfl_xor(key2, m, 64));
                }
                const bool valid = half ? vB : true;
                const uint32_t gp = half ? gB : gA;
                if (g == 0 && valid) {
                    const int rowoff = half ? rowoffB : rowoffA;
                    const bool found = key != 0x7fffffff;
                    a.oscore[gp] = (int)(half ? knownB : knownA);
                    a.oqe[gp] = found ? (key & 2047) - rowoff : -2;
                    // MODE 6 marks "one row only" in the column output (SW_TE_UNIQUE): the mirror of such a pair shares its result
                    a.ote[gp] = found ? ((key >> 11) | ((MODE == 6 && nrows == 1) ? SW_TE_UNIQUE : 0)) : -2;
                    if (a.oqe2) {   // the second answer: what the mirror of the pair reports, with the roles swapped
                        a.oqe2[gp] = found ? (key2 >> 16) - rowoff : -2;
                        a.ote2[gp] = found ? (key2 & 0xffff) : -2;
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            int score = half ? (int)(best >> 16) : (int)(best & 0xffffu);
            // the last step is nst - 1 and a lane's column in step st is st - g: the column of the last improvement is (nst - 1 - g) - age.  Exact mod 2^16
            // (a column is < 65,535) even where nst or the age wrapped.  A lane that never improved holds no column: its score is the bias, and it can
            // tie only where every lane's is, i.e. where te = -1 goes out.
            int col = -1;   // (MODE 1 reports no column)
            if constexpr (TRACK) col = (int)(((uint32_t)(nst - 1 - g) - (half ? age2 >> 16 : age2)) & 0xffffu);
#pragma unroll
            for (int m = 1; m < G; m <<= 1) {
                const int os = __shfl_xor(score, m, 64), oc = __shfl_xor(col, m, 64);
                const bool take = os > score || (os == score && oc < col);
                score = take ? os : score;
                col = take ? oc : col;
            }
            int cnt = 0, minrow = 1 << 30;
            if constexpr (TRACK) {
#pragma unroll
                for (int r = R - 1; r >= 0; r--) {
                    const int rb = half ? (int)(rowbest[r] >> 16) : (int)(rowbest[r] & 0xffffu);
                    if (rb == score) { cnt++; minrow = g * R + r; }
                }
#pragma unroll
                for (int m = 1; m < G; m <<= 1) {
                    cnt += __shfl_xor(cnt, m, 64);
                    minrow = min(minrow, __shfl_xor(minrow, m, 64));
                }
            }
            const bool valid = half ? vB : true;
            const uint32_t gp = half ? gB : gA;
            if (g == 0 && valid) {
                const int sc = score - 128;   // the reductions above compare biased values with biased values; what leaves the kernel is unbiased
                a.oscore[gp] = sc;
                if constexpr (TRACK) {
                    const int rowoff = half ? rowoffB : rowoffA;
                    int qe = -1, te = -1;
                    if (sc > 0) { te = col; qe = (cnt == 1 && sc < SW_PK_OVF) ? minrow - rowoff : -2; }
                    a.oqe[gp] = qe;
                    a.ote[gp] = te;
                }
            }
        }
    };

    start_slot();
    while (__builtin_amdgcn_ballot_w64(active) != 0) {
        if (active) {
            do_step(lst, false);
            do_step(lst + 1, true);
            lst += 2;
            if (lst >= nst) {
                finish_slot();
                start_slot();
            }
        }
    }
}

// Tasks per workgroup of a class's multi-query variant (sw_pk_kernel<.., K>), 1 = the class has none.  A variant runs K times the waves of the class's
// workgroup on K profiles, so LDS per wave stays what it is at K = 1; what decides K is that no class may hold a wave per SIMD less than at K = 1
// (profiles/multi_query_tasks/kernel_resources.txt: -Rpass-analysis=kernel-resource-usage of every variant, w waves per SIMD):
//  * G = 16 (2 waves at K = 1): K = 2 is a 4-wave workgroup, and w of them fit a CU whatever w is.  K = 4 (8 waves, for the classes whose w is even)
//    was built and measured: no faster than K = 2 at configs[1] (profiles/multi_query_tasks/README.md), so one variant per class it is.
//  * MODE 4 at R = 8, 10, 14: the K = 2 variant itself needs registers past a wave step (7 -> 6, 6 -> 5, 5 -> 4 waves): K = 1.  (16, 2): MODE 6 likewise
//    (64 -> 65 VGPRs), and the class is all but empty.
//  * G = 32: K profiles of 28-39 KB need 8-wave workgroups, and at 3 or 5 waves per SIMD (most of its classes in MODE 0 / 6) a CU would hold a wave per
//    SIMD less; its modelled loss is 3 % (MODE 0) to 7.5 % against 7-39 % at G = 16.  G = 64: one group per wave, nothing to gain.
//  * MODE 7: tb_size_kernel derives a pair's slot partner from the one-query task layout.
constexpr int sw_pk_class_queries(int G, int R, int mode) {
    if (G != 16 || R < 4) return 1;
    if (mode == 4) return (R == 8 || R == 10 || R == 14) ? 1 : 2;
    return (mode == 0 || mode == 1 || mode == 6) ? 2 : 1;
}

// kmax > 1: the class's lists are short (launch_plan) - serve sw_pk_class_queries() tasks per workgroup, if tcap (pairs per task of the class) lets the
// slots of that many tasks fit the kernel's slot table.  Returns the tasks per workgroup of the launch.
template <int MODE>
int launch_sw_pk_class_mode(int G, int R, const SwArgs &a, uint32_t n_tasks, hipStream_t s, int kmax, uint32_t tcap) {
#define UC_SW_LAUNCH(GG, RR, NW, KK)                                                                    \
    {                                                                                                   \
        const size_t lds = (size_t)KK * 2 * SW_NLET * GG * BW * 4 + 16 + (KK > 1 ? 16 * KK + 5 * SW_MQ_SLOTS : 0); \
        static PerDeviceOnce once;                                                                      \
        if (lds > 64 * 1024)                                                                            \
            once([&] { (void)hipFuncSetAttribute((const void *)sw_pk_kernel<GG, RR, MODE, NW, KK>,       \
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }); \
        SwArgs ak = a;                                                                                  \
        ak.n_tasks = n_tasks;                                                                           \
        hipLaunchKernelGGL((sw_pk_kernel<GG, RR, MODE, NW, KK>), dim3((n_tasks + KK - 1) / KK), dim3(NW * 64), lds, s, ak); \
        return KK;                                                                                      \
    }
#define UC_SW_CASE(GG, RR)                                                                              \
    if (G == GG && R == RR) {                                                                           \
        constexpr int BW = (((RR + 3) / 4) | 1);                                                        \
        /* small workgroups share one LDS profile; G = 64 with R < 14: the wave-wide classes of sparse known-score plans (table 3 of uc_sw_plan.hip) */ \
        constexpr int NW = GG == 16 ? 2 : (GG == 32 ? 4 : (RR < 14 ? 2 : 8));                           \
        constexpr int KC = sw_pk_class_queries(GG, RR, MODE);                                           \
        if constexpr (KC > 1) {                                                                         \
            const uint32_t ts = (tcap + 1) / 2;   /* slots per task at most */                          \
            /* K times the waves on K profiles: LDS per wave, and with it the waves a CU holds, stay what they are at K = 1 */ \
            if (kmax > 1 && ts <= 64 && KC * ts <= (uint32_t)SW_MQ_SLOTS) UC_SW_LAUNCH(GG, RR, NW * KC, KC) \
        }                                                                                               \
        UC_SW_LAUNCH(GG, RR, NW, 1)                                                                     \
    }
    // even R: 32-row class steps for G=16, 64 for G=32, 128 for G=64 (row padding 11.7 % -> 6.2 % at C2, tools/geom_stats.py)
    UC_SW_CASE(16, 2) UC_SW_CASE(16, 4) UC_SW_CASE(16, 6) UC_SW_CASE(16, 8) UC_SW_CASE(16, 10) UC_SW_CASE(16, 12)
    UC_SW_CASE(16, 14) UC_SW_CASE(16, 16) UC_SW_CASE(16, 18) UC_SW_CASE(16, 20) UC_SW_CASE(16, 22) UC_SW_CASE(16, 24)
    UC_SW_CASE(32, 14) UC_SW_CASE(32, 16) UC_SW_CASE(32, 18) UC_SW_CASE(32, 20) UC_SW_CASE(32, 22) UC_SW_CASE(32, 24)
    UC_SW_CASE(64, 14) UC_SW_CASE(64, 16) UC_SW_CASE(64, 18) UC_SW_CASE(64, 20) UC_SW_CASE(64, 22) UC_SW_CASE(64, 24)
    UC_SW_CASE(64, 26) UC_SW_CASE(64, 28) UC_SW_CASE(64, 30) UC_SW_CASE(64, 32)   // ~6R + 60 live registers: R = 32 still fits 256 VGPRs
    if constexpr (MODE == 4 || MODE == 6) {   // sparse plans only exist for the known-score passes
        UC_SW_CASE(64, 2) UC_SW_CASE(64, 4) UC_SW_CASE(64, 6) UC_SW_CASE(64, 8) UC_SW_CASE(64, 10) UC_SW_CASE(64, 12)
    }
#undef UC_SW_CASE
#undef UC_SW_LAUNCH
    fprintf(stderr, "unicore-cluster: no packed SW kernel for class (G=%d, R=%d)\n", G, R);
    abort();
}

// forces this translation unit's code object onto the current device (HIP loads a module lazily at the first use of one of its kernels): see preload_modules()
template <int MODE>
void preload_sw_pk_mode() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, (const void *)sw_pk_kernel<64, 14, MODE, 8>);
}

}  // namespace uc
