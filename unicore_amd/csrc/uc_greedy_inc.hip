// uc_greedy_inc.hip — stage E7 under --cluster-mode 2 (rule UC-1/G): greedy incremental clustering on the device.
// The sequential rule (uc_setcover.cpp: greedy_incremental) walks the nodes by rank - length descending, ties by ascending id - and makes every node
// that is still unassigned a representative that takes its unassigned neighbours.  Equivalently: the representatives are the lexicographically first
// maximal independent set in rank order, and every other node belongs to its representative neighbour of the SMALLEST rank.  That form runs in parallel
// rounds over a work list of undecided nodes, a wave per node like the set cover's rounds (uc_cluster_graph.hip):
//   (a) an undecided node whose lower-rank neighbours are all MEMBER becomes REP          (gi_rep_kernel)
//   (b) an undecided node with a REP neighbour becomes MEMBER, the others are kept         (gi_member_kernel: decision and compaction in one pass)
// and after ALL rounds assign[v] = the REP neighbour of the smallest rank (gi_assign_kernel): a representative of lower rank may be decided in a later
// round than one of higher rank (hub chains), so the first one seen is not the answer.  The node of the lowest rank among the undecided always decides
// (after (b) no undecided node has a REP neighbour, so its lower-rank neighbours are all MEMBER): a round without a decision is an error.  The number of
// rounds is the longest path along which the ranks ascend; a path graph of equal lengths takes n / 2, which is what the host tail below is for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_align_internal.h"

namespace uc {

constexpr uint32_t GI_UNDECIDED = 0xFFFFFFFFu;      // the "unassigned" mark sc_induced_kernel looks for: the host tail gathers on `state` as it is
constexpr uint32_t GI_MEMBER = 0u, GI_REP = 1u;

__global__ void __launch_bounds__(256) gi_key_kernel(uint32_t n, const uint32_t *len, uint64_t *key) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) key[i] = ((uint64_t)(0xFFFFFFFFu - len[i]) << 32) | i;
}
// sorted keys -> order[rank] = node, rank[node]; every node starts undecided, the first work list is the rank order
__global__ void __launch_bounds__(256) gi_rank_kernel(uint32_t n, const uint64_t *sorted, uint32_t *order, uint32_t *rank, uint32_t *state, uint32_t *work) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t v = (uint32_t)sorted[i];
        order[i] = v; rank[v] = i; work[i] = v; state[i] = GI_UNDECIDED;
    }
}
// ctr: [0] nodes in `work`, [1] new representatives, [2] new members, [3] nodes in the next work list
// (a) reads what the round before left: the only store is UNDECIDED -> REP, and a neighbour that looks at such a node is held back by either value
__global__ void __launch_bounds__(256) gi_rep_kernel(uint32_t *ctr, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *rank, uint32_t *state) {
    const uint32_t nw = ctr[0], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nw; i += gridDim.x * 4) {
        const uint32_t v = work[i], rv = rank[v];
        int held = 0;
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) { const uint32_t w = adj[e]; held |= (rank[w] < rv && state[w] != GI_MEMBER) ? 1 : 0; }
        if (!__any(held) && lane == 0) { state[v] = GI_REP; atomicAdd(&ctr[1], 1u); }
    }
}
// (b) + (c): REP is final once (a) has run, so this pass reads stable values; whoever stays undecided goes to the next work list
__global__ void __launch_bounds__(256) gi_member_kernel(uint32_t *ctr, const uint32_t *work, const uint64_t *off, const uint32_t *adj, uint32_t *state, uint32_t *next) {
    const uint32_t nw = ctr[0], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nw; i += gridDim.x * 4) {
        const uint32_t v = work[i];
        if (state[v] != GI_UNDECIDED) continue;      // a representative of this round
        int has = 0;
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) has |= state[adj[e]] == GI_REP ? 1 : 0;
        has = __any(has);
        if (lane == 0) {
            if (has) { state[v] = GI_MEMBER; atomicAdd(&ctr[2], 1u); }
            else next[atomicAdd(&ctr[3], 1u)] = v;
        }
    }
}
__global__ void gi_next_round_kernel(uint32_t *ctr) { ctr[0] = ctr[3]; ctr[1] = 0; ctr[2] = 0; ctr[3] = 0; }
// what the host finished (the nodes that were still undecided): representative or member
__global__ void __launch_bounds__(256) gi_tail_kernel(uint32_t k, const uint32_t *id, const uint32_t *rep, uint32_t *state) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < k; i += gridDim.x * 256) state[id[i]] = rep[i] ? GI_REP : GI_MEMBER;
}
__device__ __forceinline__ uint32_t gi_wave_min(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(v, o, 64); v = x < v ? x : v; }
    return v;
}
// after all rounds: a representative is its own, a member goes to its representative neighbour of the smallest rank
__global__ void __launch_bounds__(256) gi_assign_kernel(uint32_t n, const uint64_t *off, const uint32_t *adj, const uint32_t *rank, const uint32_t *order,
                                                        const uint32_t *state, uint32_t *assign, uint32_t *err) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += (uint64_t)gridDim.x * 4) {
        if (state[v] == GI_REP) { if (lane == 0) assign[v] = (uint32_t)v; continue; }
        uint32_t best = 0xFFFFFFFFu;
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) { const uint32_t w = adj[e]; if (state[w] == GI_REP) { const uint32_t r = rank[w]; best = r < best ? r : best; } }
        best = gi_wave_min(best);
        if (lane == 0) {
            if (best == 0xFFFFFFFFu) { atomicAdd(err, 1u); assign[v] = (uint32_t)v; }      // cannot happen: a member has a representative neighbour
            else assign[v] = order[best];
        }
    }
}

void Engine::greedy_inc_graph(uint32_t n, const uint32_t *h_edges, const uint32_t *dev_edges, uint64_t n_edges, uint32_t *assign) {
    PressureScope ps(*this, 1);
    UC_HIP(hipSetDevice(device));
    if (!have_db || n != hdb.n) fail(UC_ERR_ARGS, "cluster graph: mode 2 ranks the %u sequences of the resident database, not %u nodes", have_db ? hdb.n : 0u, n);
    if (!n_edges) { for (uint32_t i = 0; i < n; i++) assign[i] = i; return; }      // no edges: every node is its own representative
    const DevGraph G = build_cluster_graph(n, h_edges, dev_edges, n_edges);
    const bool timing = getenv("UC_TIMING") != nullptr;
    Timer t_rounds;
    GreedyIncScratch &S = scratch_of(*this).gi;
    S.key.reserve(n); S.key2.reserve(n); S.order.reserve(n); S.rank.reserve(n); S.state.reserve(n); S.work.reserve(n); S.work2.reserve(n);
    S.ctr.reserve(4); S.assign.reserve(n); S.err.reserve(1);
    hipLaunchKernelGGL(gi_key_kernel, grid_for(n), dim3(256), 0, stream, n, (const uint32_t *)d_len.p, S.key.p);
    rocprim_call(S.tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, S.key.p, S.key2.p, (size_t)n, 0u, 64u, stream); });
    hipLaunchKernelGGL(gi_rank_kernel, grid_for(n), dim3(256), 0, stream, n, (const uint64_t *)S.key2.p, S.order.p, S.rank.p, S.state.p, S.work.p);
    const uint32_t h_ctr[4] = {n, 0, 0, 0};
    UC_HIP(hipMemcpyAsync(S.ctr.p, h_ctr, 16, hipMemcpyHostToDevice, stream));
    UC_HIP(hipMemsetAsync(S.err.p, 0, 4, stream));
    uint32_t left = n, rounds = 0;
    bool host_tail = false;
    uint32_t *cur = S.work.p, *nxt = S.work2.p;
    while (left) {
        const dim3 gw((uint32_t)std::min<uint64_t>(((uint64_t)left + 3) / 4, 1u << 16));
        hipLaunchKernelGGL(gi_rep_kernel, gw, dim3(256), 0, stream, S.ctr.p, (const uint32_t *)cur, G.off, G.adj, (const uint32_t *)S.rank.p, S.state.p);
        hipLaunchKernelGGL(gi_member_kernel, gw, dim3(256), 0, stream, S.ctr.p, (const uint32_t *)cur, G.off, G.adj, S.state.p, nxt);
        uint32_t h[4];
        UC_HIP(hipMemcpyAsync(h, S.ctr.p, 16, hipMemcpyDeviceToHost, stream));
        hipLaunchKernelGGL(gi_next_round_kernel, dim3(1), dim3(1), 0, stream, S.ctr.p);
        UC_HIP(hipStreamSynchronize(stream));
        if (h[1] == 0) fail(UC_ERR_GENERIC, "greedy incremental: a round decided nothing with %u nodes left", left);      // cannot happen: the lowest rank always decides
        if (h[1] + h[2] + h[3] != left) fail(UC_ERR_GENERIC, "greedy incremental: %u nodes became %u + %u + %u", left, h[1], h[2], h[3]);
        left = h[3];
        std::swap(cur, nxt);
        rounds++;
        // a chain-like remainder (ranks ascending along a path) decides two nodes per round: when the rounds stop paying, the host finishes (as in the set cover)
        if (left && rounds >= 32 && h[1] + h[2] < 64) { host_tail = true; break; }
    }
    const uint32_t tail_nodes = host_tail ? left : 0;
    if (host_tail) {
        // the undecided nodes have no REP neighbour (pass (b) would have taken them), so the rule on the subgraph they induce, in the same rank order,
        // decides them exactly; their flags go back to the device before the final pass
        std::vector<uint32_t> back, e2;
        induced_subgraph(G, left, cur, S.state.p, back, e2);
        std::vector<uint32_t> sub_len(back.size()), a2(back.size()), rep(back.size());
        for (size_t i = 0; i < back.size(); i++) sub_len[i] = h_len[back[i]];      // ascending ids: ties keep their order
        cluster_graph((uint32_t)back.size(), e2.data(), e2.size() / 2, sub_len.data(), 2, a2.data());
        for (size_t i = 0; i < back.size(); i++) rep[i] = a2[i] == i ? 1u : 0u;
        S.tail_id.reserve(left); S.tail_rep.reserve(left);
        UC_HIP(hipMemcpyAsync(S.tail_id.p, back.data(), (size_t)left * 4, hipMemcpyHostToDevice, stream));
        UC_HIP(hipMemcpyAsync(S.tail_rep.p, rep.data(), (size_t)left * 4, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(gi_tail_kernel, grid_for(left), dim3(256), 0, stream, left, (const uint32_t *)S.tail_id.p, (const uint32_t *)S.tail_rep.p, S.state.p);
        UC_HIP(hipStreamSynchronize(stream));      // `back` and `rep` are read by the copies until here
    }
    const dim3 ga((uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 1u << 16));
    hipLaunchKernelGGL(gi_assign_kernel, ga, dim3(256), 0, stream, n, G.off, G.adj, (const uint32_t *)S.rank.p, (const uint32_t *)S.order.p,
                       (const uint32_t *)S.state.p, S.assign.p, S.err.p);
    uint32_t herr = 0;
    UC_HIP(hipMemcpyAsync(assign, S.assign.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipMemcpyAsync(&herr, S.err.p, 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    UC_HIP(hipGetLastError());
    if (herr) fail(UC_ERR_GENERIC, "greedy incremental: %u members without a representative neighbour", herr);
    if (timing) {
        char tail[96] = "";
        if (host_tail) snprintf(tail, sizeof tail, ", the chain-like rest (%u nodes) on the host", tail_nodes);
        fprintf(stderr, "cluster_graph_device: greedy incremental on the GPU %.2f ms in %u rounds%s\n", t_rounds.seconds() * 1e3, rounds, tail);
    }
}

void Engine::cluster_graph_dev_edges(uint32_t n, const uint32_t *dev_edges, uint64_t n_edges, uint32_t *assign) {
    if (p.cluster_mode == 0) set_cover_graph(n, nullptr, dev_edges, n_edges, assign);
    else greedy_inc_graph(n, nullptr, dev_edges, n_edges, assign);
}

void Engine::cluster_graph_device(int mode, uint32_t n, const uint32_t *h_edges, uint64_t n_edges, uint32_t *assign) {
    if (mode == 0) { set_cover_device(n, h_edges, n_edges, assign); return; }
    if (mode != 2) fail(UC_ERR_ARGS, "cluster graph: mode %d unsupported (0 = greedy set cover, 2 = greedy incremental)", mode);
    if (!have_db || n != hdb.n) fail(UC_ERR_ARGS, "cluster graph: mode 2 ranks the sequences of the resident database");
    if (n_edges >= (1ull << 31)) { cluster_graph(n, h_edges, n_edges, h_len.data(), 2, assign); return; }   // 32-bit scan positions of the graph build
    greedy_inc_graph(n, h_edges, nullptr, n_edges, assign);
}

}  // namespace uc
