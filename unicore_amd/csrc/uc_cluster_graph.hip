// uc_cluster_graph.hip - stage E7 on the device: the clustering graph and the greedy set cover.
// The accepted pairs of the gapped stage (a device or a host edge list) become a CSR graph - both directions, duplicates and self loops removed -
// that all three clustering rules start from (build_cluster_graph: this file's set cover, uc_greedy_inc.hip, uc_reassign.hip); the set cover then
// runs as parallel rounds of local maxima with the assignment of the sequential rule, and a chain-like rest is finished on the host
// (stands for Foldseek's clust --cluster-mode 0; uc_setcover.cpp is the all-host variant).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_align_internal.h"

namespace uc {

// ---- E7 graph construction on the device (the greedy cover follows below; uc_setcover.cpp is the all-host variant behind uc_setcover) ----
// both directions of every accepted pair as 64-bit keys, self loops -> all-ones (sorted last, dropped)
__global__ void __launch_bounds__(256) edge_key_kernel(uint64_t n_edges, const uint32_t *e, uint32_t n, uint64_t *key, uint32_t *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_edges; i += (uint64_t)gridDim.x * 256) {
        const uint32_t a = e[2 * i], b = e[2 * i + 1];
        if (a >= n || b >= n) { atomicAdd(bad, 1u); key[2 * i] = ~0ull; key[2 * i + 1] = ~0ull; continue; }
        key[2 * i] = a == b ? ~0ull : ((uint64_t)a << 32) | b;
        key[2 * i + 1] = a == b ? ~0ull : ((uint64_t)b << 32) | a;
    }
}
__global__ void __launch_bounds__(256) edge_uniq_kernel(uint64_t m, const uint64_t *key, uint32_t *flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256)
        flag[i] = (key[i] != ~0ull && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) edge_adj_kernel(uint64_t m, const uint64_t *key, const uint32_t *flag, const uint32_t *pos,
                                                       uint64_t *ukey, uint32_t *adj) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256)
        if (flag[i]) { ukey[pos[i]] = key[i]; adj[pos[i]] = (uint32_t)key[i]; }
}
__global__ void __launch_bounds__(256) edge_off_kernel(uint32_t n, const uint64_t *ukey, uint64_t mu, uint64_t *off) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i <= n; i += gridDim.x * 256) {
        const uint64_t want = (uint64_t)i << 32;
        uint64_t lo = 0, hi = mu;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (ukey[mid] < want) lo = mid + 1; else hi = mid; }
        off[i] = lo;
    }
}

const std::vector<uint32_t> &Engine::host_edges() {
    if (!edges_on_host) {
        UC_HIP(hipSetDevice(device));
        edges.resize(2 * n_edges_dev);
        if (n_edges_dev) UC_HIP(hipMemcpy(edges.data(), d_edges.p, 2 * n_edges_dev * 4, hipMemcpyDeviceToHost));
        edges_on_host = true;
    }
    return edges;
}

// ---- E7 on the device: the SAME greedy cover as uc_setcover.cpp (most unassigned nodes covered first, ties: smallest id), in parallel rounds ----
// The sequential rule picks the unassigned node u with the largest key (count, -id), count = 1 + unassigned neighbours.  A pick changes counts only
// within two hops THROUGH UNASSIGNED nodes (it assigns its unassigned neighbours v, which lowers the count of their unassigned neighbours w), and counts
// only ever fall.  So a node whose key is the maximum of its two-hop neighbourhood through unassigned nodes will be picked by the sequential rule with
// exactly its present count before anything near it changes: every such local maximum can be picked AT ONCE (no two of them share an unassigned
// neighbour: they would be within two hops of each other).  Rounds of (1) m1[v] = max key over the unassigned closed neighbourhood of v, (2) u is picked
// iff key(u) = max m1 over its unassigned closed neighbourhood, (3) picks take their unassigned neighbours, (4) the counts of the unassigned neighbours
// of everything newly assigned drop.  Identical assignment to the host cover (tests/test_gpu_parity.py, random graphs included); a wave per node.
constexpr uint32_t SC_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint64_t sc_key(uint32_t w, const uint32_t *assign, const uint32_t *cnt) {
    return assign[w] == SC_NONE ? ((uint64_t)cnt[w] << 32) | (uint64_t)(0xFFFFFFFFu - w) : 0ull;
}
__device__ __forceinline__ uint64_t sc_wave_max(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint64_t x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return v;
}
__global__ void __launch_bounds__(256) sc_init_kernel(uint32_t n, const uint64_t *off, uint32_t *assign, uint32_t *cnt, uint32_t *work) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        assign[i] = SC_NONE; cnt[i] = (uint32_t)(off[i + 1] - off[i]) + 1u; work[i] = i;
    }
}
// ctr: [0] nodes in `work`, [1] picks, [2] newly assigned, [3] nodes in the next work list
__global__ void __launch_bounds__(256) sc_m1_kernel(const uint32_t *ctr, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *assign,
                                                    const uint32_t *cnt, uint64_t *m1) {
    const uint32_t nw = ctr[0], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nw; i += gridDim.x * 4) {
        const uint32_t v = work[i];
        uint64_t best = 0;
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) { const uint64_t k = sc_key(adj[e], assign, cnt); best = k > best ? k : best; }
        best = sc_wave_max(best);
        const uint64_t own = sc_key(v, assign, cnt);
        if (lane == 0) m1[v] = own > best ? own : best;
    }
}
__global__ void __launch_bounds__(256) sc_pick_kernel(uint32_t *ctr, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *assign,
                                                      const uint32_t *cnt, const uint64_t *m1, uint32_t *picks) {
    const uint32_t nw = ctr[0], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nw; i += gridDim.x * 4) {
        const uint32_t u = work[i];
        uint64_t best = 0;
        for (uint64_t e = off[u] + lane; e < off[u + 1]; e += 64) {
            const uint32_t w = adj[e];
            const uint64_t k = assign[w] == SC_NONE ? m1[w] : 0ull;
            best = k > best ? k : best;
        }
        best = sc_wave_max(best);
        const uint64_t mine = m1[u];
        best = mine > best ? mine : best;
        if (lane == 0 && best == sc_key(u, assign, cnt)) picks[atomicAdd(&ctr[1], 1u)] = u;
    }
}
__global__ void __launch_bounds__(256) sc_apply_kernel(uint32_t *ctr, const uint32_t *picks, const uint64_t *off, const uint32_t *adj, uint32_t *assign, uint32_t *newly) {
    const uint32_t np = ctr[1], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < np; i += gridDim.x * 4) {
        const uint32_t u = picks[i];
        if (lane == 0) { assign[u] = u; newly[atomicAdd(&ctr[2], 1u)] = u; }
        for (uint64_t e = off[u] + lane; e < off[u + 1]; e += 64) {
            const uint32_t w = adj[e];
            if (assign[w] == SC_NONE) { assign[w] = u; newly[atomicAdd(&ctr[2], 1u)] = w; }     // no other pick of this round can reach w
        }
    }
}
__global__ void __launch_bounds__(256) sc_dec_kernel(const uint32_t *ctr, const uint32_t *newly, const uint64_t *off, const uint32_t *adj, const uint32_t *assign, uint32_t *cnt) {
    const uint32_t nn = ctr[2], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nn; i += gridDim.x * 4) {
        const uint32_t v = newly[i];
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) {
            const uint32_t w = adj[e];
            if (assign[w] == SC_NONE) atomicSub(&cnt[w], 1u);
        }
    }
}
__global__ void __launch_bounds__(256) sc_compact_kernel(uint32_t *ctr, const uint32_t *work, const uint32_t *assign, uint32_t *next) {
    const uint32_t nw = ctr[0];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nw; i += gridDim.x * 256) {
        const uint32_t v = work[i];
        if (assign[v] == SC_NONE) next[atomicAdd(&ctr[3], 1u)] = v;
    }
}
// the edges among the still-unassigned nodes of the work list (v < w once each): out == nullptr counts them, else appends them behind an atomic cursor
__global__ void __launch_bounds__(256) sc_induced_kernel(uint32_t left, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *assign,
                                                         uint32_t *out, unsigned long long *cursor) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < left; i += gridDim.x * 256) {
        const uint32_t v = work[i];
        if (assign[v] != SC_NONE) continue;
        uint32_t c = 0;
        for (uint64_t k = off[v]; k < off[(size_t)v + 1]; k++) { const uint32_t w = adj[k]; c += (w > v && assign[w] == SC_NONE) ? 1u : 0u; }
        if (!c) continue;
        const unsigned long long base = atomicAdd(cursor, (unsigned long long)c);
        if (!out) continue;
        unsigned long long o = base;
        for (uint64_t k = off[v]; k < off[(size_t)v + 1]; k++) {
            const uint32_t w = adj[k];
            if (w > v && assign[w] == SC_NONE) { out[2 * o] = v; out[2 * o + 1] = w; o++; }
        }
    }
}
__global__ void sc_next_round_kernel(uint32_t *ctr) { ctr[0] = ctr[3]; ctr[1] = 0; ctr[2] = 0; ctr[3] = 0; }

void Engine::set_cover_own_edges(uint32_t n, uint32_t *assign) {
    if (p.cluster_mode != 0) {      // --cluster-mode 2: the same three sources, the greedy incremental rule (uc_greedy_inc.hip)
        if (edges_on_host) cluster_graph_device(p.cluster_mode, n, edges.data(), edges.size() / 2, assign);
        else if (n_edges_dev >= (1ull << 31)) { const std::vector<uint32_t> &h = host_edges(); cluster_graph(n, h.data(), h.size() / 2, h_len.data(), p.cluster_mode, assign); }
        else cluster_graph_dev_edges(n, d_edges.p, n_edges_dev, assign);
        return;
    }
    if (edges_on_host) { set_cover_device(n, edges.data(), edges.size() / 2, assign); return; }
    if (n_edges_dev >= (1ull << 31)) { const std::vector<uint32_t> &h = host_edges(); set_cover(n, h.data(), h.size() / 2, assign); return; }
    set_cover_graph(n, nullptr, d_edges.p, n_edges_dev, assign);
}

void Engine::set_cover_device(uint32_t n, const uint32_t *h_edges, uint64_t n_edges, uint32_t *assign) {
    if (n_edges >= (1ull << 31)) { set_cover(n, h_edges, n_edges, assign); return; }   // 32-bit scan positions below
    set_cover_graph(n, h_edges, nullptr, n_edges, assign);
}

// the graph (CSR, both directions, duplicates and self loops removed) on the device from a host or a device edge list (n_edges > 0): the step
// both clustering rules start from.  The arrays live in the engine's scratch and stay valid until the next graph build
DevGraph Engine::build_cluster_graph(uint32_t n, const uint32_t *h_edges, const uint32_t *dev_edges, uint64_t n_edges) {
    Timer t_graph;
    AlignScratch &A = scratch_of(*this);
    const uint64_t m = 2 * n_edges;
    DevBuf<uint32_t> &d_e = A.sc.e, &flag = A.sc.flag, &pos = A.sc.pos, &d_adj = A.sc.dadj, &bad = A.sc.bad;
    DevBuf<uint64_t> &key = A.sc.key, &key2 = A.sc.key2, &ukey = A.sc.ukey, &d_off = A.sc.doff;
    DevBuf<char> &tmp = A.sc.tmp;
    key.reserve(m); key2.reserve(m); flag.reserve(m); pos.reserve(m); bad.reserve(1); d_off.reserve((size_t)n + 1);
    const uint32_t *e_in = dev_edges;
    if (!e_in) {
        d_e.reserve(m);
        UC_HIP(hipMemcpyAsync(d_e.p, h_edges, m * 4, hipMemcpyHostToDevice, stream));
        e_in = d_e.p;
    }
    UC_HIP(hipMemsetAsync(bad.p, 0, 4, stream));
    hipLaunchKernelGGL(edge_key_kernel, grid_for(n_edges), dim3(256), 0, stream, n_edges, e_in, n, key.p, bad.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, key.p, key2.p, (size_t)m, 0u, 64u, stream); });
    hipLaunchKernelGGL(edge_uniq_kernel, grid_for(m), dim3(256), 0, stream, m, key2.p, flag.p);
    const uint32_t mu = compact(*this, tmp, flag.p, pos.p, (uint32_t)m);
    uint32_t hbad = 0;
    UC_HIP(hipMemcpy(&hbad, bad.p, 4, hipMemcpyDeviceToHost));
    if (hbad) fail(UC_ERR_ARGS, "set cover: %u edges with an endpoint out of range", hbad);
    ukey.reserve(std::max<uint32_t>(mu, 1)); d_adj.reserve(std::max<uint32_t>(mu, 1));
    hipLaunchKernelGGL(edge_adj_kernel, grid_for(m), dim3(256), 0, stream, m, key2.p, flag.p, pos.p, ukey.p, d_adj.p);
    hipLaunchKernelGGL(edge_off_kernel, grid_for((uint64_t)n + 1), dim3(256), 0, stream, n, ukey.p, (uint64_t)mu, d_off.p);
    UC_HIP(hipGetLastError());
    if (getenv("UC_TIMING")) { UC_HIP(hipStreamSynchronize(stream)); fprintf(stderr, "set_cover_device: graph on the GPU %.2f ms\n", t_graph.seconds() * 1e3); }
    return DevGraph{d_off.p, d_adj.p, mu};
}

// the subgraph the still-undecided nodes (mark[v] == SC_NONE) of the work list induce, for a host finish: their ids ascending (`back`) and the edges
// among them in that numbering (`e2`, each once), gathered on the device (count pass, then an append pass; the order of the edge list does not matter)
void Engine::induced_subgraph(const DevGraph &G, uint32_t left, const uint32_t *d_work, const uint32_t *d_mark, std::vector<uint32_t> &back, std::vector<uint32_t> &e2) {
    DevBuf<unsigned long long> ecnt;
    ecnt.reserve(1);
    UC_HIP(hipMemsetAsync(ecnt.p, 0, 8, stream));
    hipLaunchKernelGGL(sc_induced_kernel, grid_for(left), dim3(256), 0, stream, left, d_work, G.off, G.adj, d_mark, (uint32_t *)nullptr, ecnt.p);
    unsigned long long ne2 = 0;
    UC_HIP(hipMemcpyAsync(&ne2, ecnt.p, 8, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    DevBuf<uint32_t> de2;
    de2.reserve(2 * std::max<unsigned long long>(ne2, 1));
    UC_HIP(hipMemsetAsync(ecnt.p, 0, 8, stream));
    if (ne2) hipLaunchKernelGGL(sc_induced_kernel, grid_for(left), dim3(256), 0, stream, left, d_work, G.off, G.adj, d_mark, de2.p, ecnt.p);
    back.resize(left); e2.resize(2 * (size_t)ne2);
    UC_HIP(hipMemcpyAsync(back.data(), d_work, (size_t)left * 4, hipMemcpyDeviceToHost, stream));
    if (ne2) UC_HIP(hipMemcpyAsync(e2.data(), de2.p, 2 * (size_t)ne2 * 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    UC_HIP(hipGetLastError());
    std::sort(back.begin(), back.end());                                   // ids keep their order: so do the ties
    auto sub = [&](uint32_t v) { return (uint32_t)(std::lower_bound(back.begin(), back.end(), v) - back.begin()); };
    for (uint32_t &x : e2) x = sub(x);
}

// the graph on the device (build_cluster_graph), then the greedy cover on the device as well (parallel rounds of local maxima: the host cover's
// assignment, uc_setcover.cpp, exactly)
void Engine::set_cover_graph(uint32_t n, const uint32_t *h_edges, const uint32_t *dev_edges, uint64_t n_edges, uint32_t *assign) {
    PressureScope ps(*this, 1);
    UC_HIP(hipSetDevice(device));
    AlignScratch &A = scratch_of(*this);
    if (n_edges) {
        const DevGraph G = build_cluster_graph(n, h_edges, dev_edges, n_edges);
        const uint64_t *d_off = G.off;
        const uint32_t *d_adj = G.adj;
        const bool timing = getenv("UC_TIMING") != nullptr;
        // the greedy cover itself, on the device too (parallel rounds, see above): neither the adjacency (2 x edges x 4 bytes) nor the serial
        // host sweep — rank 0's Amdahl term of an N-GPU pass — is left; only the assignment comes back
        Timer t_greedy;
        DevBuf<uint32_t> &d_assign = A.sc.assign, &d_cnt = A.sc.cnt, &w0 = A.sc.work, &w1 = A.sc.work2, &picks = A.sc.picks, &newly = A.sc.newly, &ctr = A.sc.ctr;
        DevBuf<uint64_t> &m1 = A.sc.m1;
        d_assign.reserve(n); d_cnt.reserve(n); w0.reserve(n); w1.reserve(n); picks.reserve(n); newly.reserve(n); ctr.reserve(4); m1.reserve(n);
        hipLaunchKernelGGL(sc_init_kernel, grid_for(n), dim3(256), 0, stream, n, d_off, d_assign.p, d_cnt.p, w0.p);
        const uint32_t h_ctr[4] = {n, 0, 0, 0};
        UC_HIP(hipMemcpyAsync(ctr.p, h_ctr, 16, hipMemcpyHostToDevice, stream));
        uint32_t left = n, rounds = 0;
        bool host_tail = false;
        uint32_t *cur = w0.p, *nxt = w1.p;
        while (left) {
            const dim3 gw((uint32_t)std::min<uint64_t>(((uint64_t)left + 3) / 4, 1u << 16));
            hipLaunchKernelGGL(sc_m1_kernel, gw, dim3(256), 0, stream, (const uint32_t *)ctr.p, (const uint32_t *)cur, d_off, d_adj, d_assign.p, d_cnt.p, m1.p);
            hipLaunchKernelGGL(sc_pick_kernel, gw, dim3(256), 0, stream, ctr.p, (const uint32_t *)cur, d_off, d_adj, d_assign.p, d_cnt.p, m1.p, picks.p);
            hipLaunchKernelGGL(sc_apply_kernel, gw, dim3(256), 0, stream, ctr.p, (const uint32_t *)picks.p, d_off, d_adj, d_assign.p, newly.p);
            hipLaunchKernelGGL(sc_dec_kernel, gw, dim3(256), 0, stream, (const uint32_t *)ctr.p, (const uint32_t *)newly.p, d_off, d_adj, d_assign.p, d_cnt.p);
            hipLaunchKernelGGL(sc_compact_kernel, grid_for(left), dim3(256), 0, stream, ctr.p, (const uint32_t *)cur, d_assign.p, nxt);
            uint32_t h[4];
            UC_HIP(hipMemcpyAsync(h, ctr.p, 16, hipMemcpyDeviceToHost, stream));
            hipLaunchKernelGGL(sc_next_round_kernel, dim3(1), dim3(1), 0, stream, ctr.p);
            UC_HIP(hipStreamSynchronize(stream));
            if (h[1] == 0) fail(UC_ERR_GENERIC, "set cover: a round picked nothing with %u nodes left", left);    // cannot happen: the global maximum is always a local one
            left = h[3];
            std::swap(cur, nxt);
            rounds++;
            // Family graphs finish in a handful of rounds; a chain-like remainder (equal counts, ids ascending along a path) gives ONE pick per round -
            // n / 3 rounds of six launches and a host synchronisation each.  When the rounds stop paying, the rest - the greedy cover of
            // the subgraph the unassigned nodes induce, which is all the sequential rule still looks at - is finished by the host cover.
            if (left && rounds >= 32 && h[1] < 64) { host_tail = true; break; }
        }
        UC_HIP(hipMemcpyAsync(assign, d_assign.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        UC_HIP(hipStreamSynchronize(stream));
        UC_HIP(hipGetLastError());
        if (host_tail) {
            // r06: only the subgraph the `left` unassigned nodes induce goes to the host - their ids and the edges among them - not the whole
            // adjacency (4 B x 10^9 entries over PCIe plus an O(n) scan at nominal sizes, however few nodes were left)
            std::vector<uint32_t> back, e2;
            induced_subgraph(G, left, cur, d_assign.p, back, e2);
            std::vector<uint32_t> a2(back.size());
            set_cover((uint32_t)back.size(), e2.data(), e2.size() / 2, a2.data());
            for (size_t i = 0; i < back.size(); i++) assign[back[i]] = back[a2[i]];
        }
        if (timing) fprintf(stderr, "set_cover_device: greedy cover on the GPU %.2f ms in %u rounds%s\n", t_greedy.seconds() * 1e3, rounds,
                            host_tail ? ", the chain-like rest on the host" : "");
        return;
    }
    for (uint32_t i = 0; i < n; i++) assign[i] = i;      // no edges: every node is its own representative
}

void preload_cluster_graph_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)edge_key_kernel); }
}  // namespace uc
