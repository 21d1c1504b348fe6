// h-hop subgraph extraction, node sampling, induced-subgraph CSR build and batching on gfx950.
// Replaces Subgraphs.generate_subgraph / generate_subgraph_link_pred (sdp.py:295-346) and
// dgl.batch (sdp.py:399-406).  One workgroup per subgraph; the membership set is an LDS bitmap
// over the parent graph's nodes, so the node list comes out in ascending order for free and
// local ids are prefix popcounts.  Edge lists are read from HBM coalesced (wave per frontier node).
#include <algorithm>
#include <initializer_list>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <mutex>
#include <type_traits>
#include "gm_internal.h"
#include "gm_devutil.h"      // lowbias32, sample_salt; wld / wst: the bitmap words in LDS (G = false) or in the workgroup's slab of HBM (G = true)

#define EX_BLOCK 512
#define EX_WAVES (EX_BLOCK / GM_WAVE)

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <bool G> __device__ __forceinline__ bool bit_test(const uint32_t* bm, int v) { return (wld<G>(&bm[v >> 5]) >> (v & 31)) & 1u; }
__device__ __forceinline__ void bit_set(uint32_t* bm, int v) { atomicOr(&bm[v >> 5], 1u << (v & 31)); }
// The per-word prefix counts are 16-bit where a subgraph holds fewer than 65,536 nodes and the bitmaps live in LDS (PT = uint16_t; round 6): with the
// 21-KiB membership bitmap of a 169 k-node parent that is 35 instead of 45 KiB per workgroup -- four resident workgroups per CU instead of three.
template <bool G, typename PT> __device__ __forceinline__ int pref_ld(const PT* p) {
    if constexpr (sizeof(PT) == 4) return (int)wld<G>(reinterpret_cast<const uint32_t*>(p)); else return (int)*p;
}
template <bool G, typename PT> __device__ __forceinline__ int bit_rank(const uint32_t* bm, const PT* pref, int v) {
    return pref_ld<G, PT>(&pref[v >> 5]) + __popc(wld<G>(&bm[v >> 5]) & ((1u << (v & 31)) - 1u));
}

// Exclusive scan of part[0..EX_BLOCK) in LDS by wave 0; returns the total through *total (LDS).
__device__ __forceinline__ void scan_partials(int* part, int* total) {
    __syncthreads();
    if (threadIdx.x < GM_WAVE) {
        const int l = threadIdx.x;
        constexpr int PER = EX_BLOCK / GM_WAVE;
        int loc[PER], s = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { loc[k] = s; s += part[l * PER + k]; }
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(inc, o, 64); if (l >= o) inc += t; }
        const int base = inc - s;
#pragma unroll
        for (int k = 0; k < PER; ++k) part[l * PER + k] = base + loc[k];
        if (l == 63) *total = inc;
    }
    __syncthreads();
}

// pref[w] = number of set bits in seen[0..w); returns the total.
template <bool G, typename PT>
__device__ __forceinline__ int bitmap_prefix(const uint32_t* seen, PT* pref, int W, int* part, int* total) {
    const int chunk = (W + EX_BLOCK - 1) / EX_BLOCK;
    const int w0 = threadIdx.x * chunk, w1 = min(W, w0 + chunk);
    int s = 0;
    for (int w = w0; w < w1; ++w) s += __popc(wld<G>(&seen[w]));
    part[threadIdx.x] = s;
    scan_partials(part, total);
    int run = part[threadIdx.x];
    for (int w = w0; w < w1; ++w) {
        if constexpr (sizeof(PT) == 4) wst<G>(reinterpret_cast<uint32_t*>(&pref[w]), (uint32_t)run); else pref[w] = (PT)run;
        run += __popc(wld<G>(&seen[w]));
    }
    __syncthreads();
    return *total;
}

struct ExStore {
    const int64_t* node_off;
    const int64_t* in_ptr; const int32_t* in_idx;
    const int64_t* out_ptr; const int32_t* out_idx;
    int sym;       // the out-CSR is element for element the in-CSR (an undirected graph stored in both directions, rows ascending): the by-source
                   // CSR of an induced subgraph then IS its by-destination CSR, so the adjacency lists are walked once instead of twice
};

// Adjacency walks are latency chains (row bounds -> neighbour ids -> bitmap word), so a wave takes EIGHT nodes at a time, one per group of eight
// lanes (the median parent degree is below 16), two neighbour loads in flight per lane; nodes with more than EX_BIG_DEG neighbours are left to a
// second pass in which a whole wave walks one node (a hub in one group would stall the other seven).
#define EX_GL 8
#define EX_GROUPS (GM_WAVE / EX_GL)
#define EX_BIG_DEG 256
#define EX_INFL 4          // neighbour loads in flight per lane (round 6: 2 before -- a node of 17..32 neighbours took two dependent round trips, now one)
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
    for (int o = EX_GL / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Target-link masking (GM_LINK_MASK_TARGET): a row drops ONE neighbour id, in its in-list and its out-list alike -- the other centre on the two centre
// rows (all parallel copies; i == j: the centre's self loops), nothing (-1, no node id) on every other row.  The count pass (k_nodes) and the fill pass
// (k_fill) take the id from this one function and apply it as `inside && u != excl` in all four walkers: indptr is the scan of the counted degrees and
// the fill writes at those offsets.  MASK is a template flag of the two kernels and of the walkers: it changes no signature, and without it the
// comparison and `excl` are compiled out.
__device__ __forceinline__ int mask_excl(int v, int ci, int cj) { return v == ci ? cj : (v == cj ? ci : -1); }
// number of neighbours of v (list ptr/idx) inside the bitmap; the eight lanes of a group call it together (gl = lane within the group; excl: per group)
template <bool G, bool MASK = false>
__device__ __forceinline__ int group_count(const int64_t a, const int64_t b, const int32_t* idx, const uint32_t* seen, int gl, int excl = -1) {
    int c = 0;
    for (int64_t q = a + gl; __any(q < b); q += EX_INFL * EX_GL) {
        int u[EX_INFL];
#pragma unroll
        for (int k = 0; k < EX_INFL; ++k) u[k] = q + k * EX_GL < b ? idx[q + k * EX_GL] : -1;
#pragma unroll
        for (int k = 0; k < EX_INFL; ++k) if (u[k] >= 0 && (!MASK || u[k] != excl)) c += bit_test<G>(seen, u[k]);
    }
    return group_sum(c);
}

// Hub nodes (more than EX_BIG_DEG neighbours: thousands in a preferential-attachment parent, and every 2-hop neighbourhood holds dozens of them --
// most of a subgraph's walk volume) are walked by a whole wave, EX_WINFL x 64 neighbour ids in flight (round 6: 64 before, a round trip per 64 ids).
#define EX_WINFL 4
// Marks every in-neighbour of v (graph-local id) in `seen`; called by a whole wave.
__device__ __forceinline__ void wave_mark_preds(const ExStore& S, int64_t base, int v, uint32_t* seen, int lane) {
    const int64_t p0 = S.in_ptr[base + v], p1 = S.in_ptr[base + v + 1];
    for (int64_t q = p0 + lane; q < p1; q += EX_WINFL * GM_WAVE) {
        int u[EX_WINFL];
#pragma unroll
        for (int k = 0; k < EX_WINFL; ++k) u[k] = q + k * GM_WAVE < p1 ? S.in_idx[q + k * GM_WAVE] : -1;
#pragma unroll
        for (int k = 0; k < EX_WINFL; ++k) if (u[k] >= 0) bit_set(seen, u[k]);
    }
}
// neighbours of a hub node (list [a, b) of idx) inside the bitmap, per lane (the caller adds the lanes up; excl: wave-uniform)
template <bool G, bool MASK = false>
__device__ __forceinline__ int wave_count(const int64_t a, const int64_t b, const int32_t* idx, const uint32_t* seen, int lane, int excl = -1) {
    int c = 0;
    for (int64_t q = a + lane; q < b; q += EX_WINFL * GM_WAVE) {
        int u[EX_WINFL];
#pragma unroll
        for (int k = 0; k < EX_WINFL; ++k) u[k] = q + k * GM_WAVE < b ? idx[q + k * GM_WAVE] : -1;
#pragma unroll
        for (int k = 0; k < EX_WINFL; ++k) if (u[k] >= 0 && (!MASK || u[k] != excl)) c += bit_test<G>(seen, u[k]);
    }
    return c;
}

// The h-hop in-neighbour expansion (H = 1, 2, 3) rooted at `root`, into `seen`; called by the whole workgroup, complete (all bits visible) on return.
// `xbm` (NEEDX) is the `expanded` bitmap: a set bit means "every in-neighbour of this node is already in `seen`".  That does not depend on the root,
// so the two roots of a symmetric pair share it: what the first root expanded the second one skips.  `big` / `nbig`: the hub list of hop 2 (this
// root's; *nbig is zero on entry).
template <bool G, bool NEEDX>
__device__ __forceinline__ void expand_root(const ExStore& S, const int64_t base, const int root, const int H, uint32_t* seen, uint32_t* xbm,
                                            int* big, int* nbig, const int tid, const int lane, const int wave) {
    const int64_t p0 = S.in_ptr[base + root], p1 = S.in_ptr[base + root + 1];
    if (tid == 0) { bit_set(seen, root); if (NEEDX) bit_set(xbm, root); }
    for (int64_t q = p0 + tid; q < p1; q += EX_BLOCK) bit_set(seen, S.in_idx[q]);          // hop 1 (sdp.py:301,305,308)
    __syncthreads();
    if (H >= 2) {                                                                         // hop 2 (sdp.py:302,309)
        // eight frontier nodes per wave at a time; frontier hubs go to the list in `part` and get a whole wave each afterwards
        const int grp = lane / EX_GL, gl = lane % EX_GL;
        for (int64_t q0 = p0 + (int64_t)wave * EX_GROUPS; q0 < p1; q0 += (int64_t)EX_WAVES * EX_GROUPS) {
            const int64_t q = q0 + grp;
            int v = -1; int64_t a = 0, b = 0;
            if (q < p1) {
                v = S.in_idx[q];
                int first = 1;
                if constexpr (NEEDX) {
                    first = 0;
                    if (gl == 0) { const uint32_t bit = 1u << (v & 31); first = !(atomicOr(&xbm[v >> 5], bit) & bit); }
                    first = __shfl(first, grp * EX_GL, 64);
                }
                if (first) { a = S.in_ptr[base + v]; b = S.in_ptr[base + v + 1]; }
                if (b - a > EX_BIG_DEG) {
                    int slot = EX_BLOCK;
                    if (gl == 0) slot = atomicAdd(nbig, 1);
                    slot = __shfl(slot, grp * EX_GL, 64);
                    if (slot < EX_BLOCK) { if (gl == 0) big[slot] = v; b = a; }      // (list full: the group walks it itself)
                }
            }
            for (int64_t r = a + gl; __any(r < b); r += EX_INFL * EX_GL) {
                int u[EX_INFL];
#pragma unroll
                for (int k = 0; k < EX_INFL; ++k) u[k] = r + k * EX_GL < b ? S.in_idx[r + k * EX_GL] : -1;
#pragma unroll
                for (int k = 0; k < EX_INFL; ++k) if (u[k] >= 0) bit_set(seen, u[k]);
            }
        }
        __syncthreads();
        const int nb = min(*nbig, EX_BLOCK);
        for (int k = wave; k < nb; k += EX_WAVES) wave_mark_preds(S, base, big[k], seen, lane);
        __syncthreads();
    }
    if (H >= 3) {                                                                         // hop 3 (sdp.py:310)
        for (int64_t q = p0 + wave; q < p1; q += EX_WAVES) {
            const int v = S.in_idx[q];
            const int64_t a = S.in_ptr[base + v], b = S.in_ptr[base + v + 1];
            for (int64_t r = a; r < b; r += GM_WAVE) {
                int u = -1, first = 0;
                if (r + lane < b) {
                    u = S.in_idx[r + lane];
                    const uint32_t bit = 1u << (u & 31);
                    first = !(atomicOr(&xbm[u >> 5], bit) & bit);
                }
                unsigned long long m = __ballot(first);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    wave_mark_preds(S, base, __shfl(u, src, 64), seen, lane);
                }
            }
        }
        __syncthreads();
    }
}

// The walk over the ns rows of a subgraph (nodes[], ascending) that the count pass (k_nodes) and the fill pass (k_fill) share; called by the whole
// workgroup.  Eight rows per wave at a time, one per group of eight lanes (grp, gl: a lane's group and its place in it, the caller's own values);
// rows with more than EX_BIG_DEG neighbours in either list go to big[] (*nbig of them, zeroed here) and get a whole wave each after a barrier.
// The walk of a batch of eight rows is a chain node id -> row bounds -> neighbour ids -> bitmap word.  The first two links are taken off the chain
// (round 6): the node ids are fetched TWO batches ahead and the row bounds ONE batch ahead -- with OFFS also the rows' output offsets, off_i[r] and
// off_o[r] -- so an iteration issues three independent groups of loads and waits one round trip instead of three.
//   batch(have, later, r, v, ia, ib, oa, ob, pi, po): every lane of the wave, per batch.  have: the group has a row, r, of node v (else v = -1);
//       later: it went to big[].  [ia, ib) / [oa, ob): its in- / out-list, empty without a row or with `later`; pi / po: the offsets (0 without OFFS).
//   hub(r, v): every lane of a wave, per row of big[].  A symmetric parent (S.sym) has its out-lists left alone: oa == ob == 0.
template <bool OFFS, typename Batch, typename Hub>
__device__ __forceinline__ void walk_rows(const ExStore& S, const int64_t base, const int32_t* nodes, const int ns, const int32_t* off_i, const int32_t* off_o,
                                          int* big, int* nbig, const int tid, const int wave, const int grp, const int gl, Batch batch, Hub hub) {
    if (tid == 0) *nbig = 0;
    __syncthreads();
    constexpr int RSTEP = EX_WAVES * EX_GROUPS;
    int r = wave * EX_GROUPS + grp;
    int v1 = r < ns ? nodes[r] : -1;                                              // node of the NEXT batch
    int v2 = r + RSTEP < ns ? nodes[r + RSTEP] : -1;                              // ... of the one after
    int64_t nia = 0, nib = 0, noa = 0, nob = 0; int npi = 0, npo = 0;
    if (v1 >= 0) {
        nia = S.in_ptr[base + v1]; nib = S.in_ptr[base + v1 + 1]; if constexpr (OFFS) npi = off_i[r];
        if (!S.sym) { noa = S.out_ptr[base + v1]; nob = S.out_ptr[base + v1 + 1]; if constexpr (OFFS) npo = off_o[r]; }
    }
    for (int r0 = wave * EX_GROUPS; r0 < ns; r0 += RSTEP, r += RSTEP) {
        int64_t ia = nia, ib = nib, oa = noa, ob = nob; const int pi = npi, po = npo;
        const int v = v1;
        const bool have = v >= 0;
        v1 = v2;
        v2 = r + 2 * RSTEP < ns ? nodes[r + 2 * RSTEP] : -1;
        nia = nib = noa = nob = 0; npi = npo = 0;
        if (v1 >= 0) {
            nia = S.in_ptr[base + v1]; nib = S.in_ptr[base + v1 + 1]; if constexpr (OFFS) npi = off_i[r + RSTEP];
            if (!S.sym) { noa = S.out_ptr[base + v1]; nob = S.out_ptr[base + v1 + 1]; if constexpr (OFFS) npo = off_o[r + RSTEP]; }
        }
        bool later = false;
        if (have) {
            if (ib - ia > EX_BIG_DEG || ob - oa > EX_BIG_DEG) {
                int slot = EX_BLOCK;
                if (gl == 0) slot = atomicAdd(nbig, 1);
                slot = __shfl(slot, grp * EX_GL, 64);
                if (slot < EX_BLOCK) { if (gl == 0) big[slot] = r; later = true; ia = ib = oa = ob = 0; }      // (list full: the group walks it itself)
            }
        }
        batch(have, later, r, v, ia, ib, oa, ob, pi, po);
    }
    __syncthreads();
    const int nb = min(*nbig, EX_BLOCK);
    for (int k = wave; k < nb; k += EX_WAVES) { const int r = big[k]; hub(r, nodes[r]); }
}

// Phase A: node set (BFS or given), sampling, sorted node list, induced in/out degrees.
// P16: 16-bit prefix words (LDS bitmaps, subgraphs below 65,536 nodes).  NEEDX: keep the `expanded` bitmap that de-duplicates frontier expansions -- needed from
// the third hop on (a hop-2 node is reached through many hop-1 nodes); with two hops it only catches parallel edges of the centre, and without it the
// region behind `seen` shrinks to the 16-bit prefix words.
// SYM: pairs in GM_LINK_SYMMETRIC mode -- h hops around BOTH endpoints (link != 0 then); without it a pair is the reference's: i side two hops, j side one.
// MASK: the induced degrees are those without the target link (the node set above them is the unmasked one: BFS, sampling and node list do not look at
// the flag).  Masked and unmasked instantiations take the same arguments.
template <bool G, bool P16 = false, bool NEEDX = true, bool SYM = false, bool MASK = false>
__global__ __launch_bounds__(EX_BLOCK) void k_nodes(ExStore S, const gm_seed_t* seeds, int n_seeds, int h, int sample_n,
                                                    uint64_t rng_seed, int link, const int32_t* given, const int64_t* given_off,
                                                    int cap, int32_t* nodes_slab, int32_t* degi_slab, int32_t* dego_slab,
                                                    int32_t* n_sub, int32_t* e_sub, int Wmax, uint32_t* gbits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* seen = G ? gbits + (size_t)blockIdx.x * 2 * Wmax : lds;
    static_assert(!(G && P16), "16-bit prefix words live in LDS");
    typedef typename std::conditional<P16, uint16_t, uint32_t>::type PT;
    uint32_t* xbm = seen + Wmax;              // the `expanded` bitmap of the BFS (NEEDX); the same region holds the prefix words afterwards
    PT* pref = reinterpret_cast<PT*>(xbm);
    const int PW = (P16 && !NEEDX) ? (Wmax + 1) / 2 : Wmax;      // words of that region
    int* part = (int*)(G ? lds : lds + Wmax + PW);      // [EX_BLOCK]
    uint32_t* hist = (uint32_t*)(part + EX_BLOCK);   // [256]
    int* sc = (int*)(hist + 256);             // scalars: 0 total, 1 kk, 2 prefix, 3 edge count in, 4 edge count out
    const int seed = blockIdx.x;
    if (seed >= n_seeds) return;
    const int g = seeds[seed].graph, ci = seeds[seed].i, cj = link ? seeds[seed].j : -1;
    const int64_t base = S.node_off[g];
    const int n = (int)(S.node_off[g + 1] - base);
    const int W = (n + 31) >> 5;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;

    for (int w = tid; w < W; w += EX_BLOCK) { wst<G>(&seen[w], 0u); if (NEEDX) wst<G>(&xbm[w], 0u); }
    if (tid < 8) sc[tid] = 0;
    __syncthreads();
    if (given) {
        const int64_t a = given_off[seed], b = given_off[seed + 1];
        for (int64_t k = a + tid; k < b; k += EX_BLOCK) bit_set(seen, given[k]);
        __syncthreads();
    } else {
        const int H = SYM ? h : (link ? 2 : h);
        int* big = part; int* nbig = &sc[5];
        expand_root<G, NEEDX>(S, base, ci, H, seen, xbm, big, nbig, tid, lane, wave);
        if constexpr (SYM) {                                                                  // j side: the same h hops
            if (tid == 0) *nbig = 0;                                                          // (the hub list is per root; every wave is past its last read of it)
            __syncthreads();
            expand_root<G, NEEDX>(S, base, cj, H, seen, xbm, big, nbig, tid, lane, wave);
        } else if (link) {                                                                    // j side: 1 hop only (sdp.py:331-333)
            if (tid == 0) bit_set(seen, cj);
            const int64_t a = S.in_ptr[base + cj], b = S.in_ptr[base + cj + 1];
            for (int64_t q = a + tid; q < b; q += EX_BLOCK) bit_set(seen, S.in_idx[q]);
            __syncthreads();
        }
        // ---- count, and sample if above the threshold (strict '>' at sdp.py:312,337)
        int c = 0;
        for (int w = tid; w < W; w += EX_BLOCK) c += __popc(wld<G>(&seen[w]));
        c = wave_sum(c);
        if (lane == 0) atomicAdd(&sc[0], c);
        __syncthreads();
        const int count = sc[0];
        __syncthreads();
        if (count > sample_n) {
            // keep the sample_n nodes with the smallest key(node) = lowbias32(node ^ salt): 4-pass radix select.
            const uint32_t salt = sample_salt(rng_seed, g, ci, cj);
            if (tid == 0) { sc[1] = sample_n; sc[2] = 0; }
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                for (int k = tid; k < 256; k += EX_BLOCK) hist[k] = 0;
                __syncthreads();
                const uint32_t prefix = (uint32_t)sc[2];
                for (int w = tid; w < W; w += EX_BLOCK) {
                    uint32_t bits = wld<G>(&seen[w]);
                    while (bits) {
                        const int b = __ffs(bits) - 1; bits &= bits - 1;
                        const uint32_t key = lowbias32((uint32_t)(w * 32 + b) ^ salt);
                        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                    }
                }
                __syncthreads();
                if (tid == 0) {
                    int kk = sc[1], d = 0;
                    while (d < 255 && (int)hist[d] < kk) { kk -= (int)hist[d]; ++d; }
                    sc[1] = kk; sc[2] = (int)(prefix | ((uint32_t)d << shift));
                }
                __syncthreads();
            }
            const uint32_t tau = (uint32_t)sc[2];
            for (int w = tid; w < W; w += EX_BLOCK) {
                uint32_t bits = wld<G>(&seen[w]), keep = 0;
                while (bits) {
                    const int b = __ffs(bits) - 1; bits &= bits - 1;
                    if (lowbias32((uint32_t)(w * 32 + b) ^ salt) <= tau) keep |= 1u << b;
                }
                wst<G>(&seen[w], keep);
            }
            __syncthreads();
            if (tid == 0) { bit_set(seen, ci); if (cj >= 0) bit_set(seen, cj); }   // np.unique(np.append(., centres))
            __syncthreads();
        }
    }
    // ---- ascending node list + local-id prefix
    const int ns = bitmap_prefix<G, PT>(seen, pref, W, part, &sc[0]);
    if (ns > cap) { if (tid == 0) { n_sub[seed] = -ns; e_sub[seed] = 0; } return; }   // host reports the error
    int32_t* nodes = nodes_slab + (int64_t)seed * cap;
    for (int w = tid; w < W; w += EX_BLOCK) {
        uint32_t bits = wld<G>(&seen[w]);
        int r = pref_ld<G, PT>(&pref[w]);
        while (bits) { const int b = __ffs(bits) - 1; bits &= bits - 1; nodes[r++] = w * 32 + b; }
    }
    __syncthreads();
    // ---- induced in/out degree of every selected node (walk_rows: eight nodes per wave at a time, hubs by a whole wave afterwards)
    {
        const int grp = lane / EX_GL, gl = lane % EX_GL;
        int ein = 0, eout = 0;
        int32_t* degi = degi_slab + (int64_t)seed * cap; int32_t* dego = dego_slab + (int64_t)seed * cap;
        walk_rows<false>(S, base, nodes, ns, nullptr, nullptr, part, &sc[5], tid, wave, grp, gl,
            [&](bool have, bool later, int r, int v, int64_t ia, int64_t ib, int64_t oa, int64_t ob, int, int) {
                int excl = -1;
                if constexpr (MASK) excl = mask_excl(v, ci, cj);      // (v < 0: a group without a row, and ci, cj >= 0)
                const int ci_ = group_count<G, MASK>(ia, ib, S.in_idx, seen, gl, excl);
                const int co_ = S.sym ? ci_ : group_count<G, MASK>(oa, ob, S.out_idx, seen, gl, excl);
                if (have && gl == 0 && !later) { degi[r] = ci_; dego[r] = co_; ein += ci_; eout += co_; }      // (later: its degrees come from the second pass)
            },
            [&](int r, int v) {
                int ci_ = 0, co_ = 0;
                int excl = -1;
                if constexpr (MASK) excl = mask_excl(v, ci, cj);
                ci_ = wave_count<G, MASK>(S.in_ptr[base + v], S.in_ptr[base + v + 1], S.in_idx, seen, lane, excl);
                if (!S.sym) co_ = wave_count<G, MASK>(S.out_ptr[base + v], S.out_ptr[base + v + 1], S.out_idx, seen, lane, excl);
                ci_ = wave_sum(ci_); co_ = S.sym ? ci_ : wave_sum(co_);
                if (lane == 0) { degi[r] = ci_; dego[r] = co_; ein += ci_; eout += co_; }
            });
        if (ein | eout) { atomicAdd(&sc[3], ein); atomicAdd(&sc[4], eout); }
    }
    __syncthreads();
    if (tid == 0) { n_sub[seed] = ns; e_sub[seed] = (sc[3] == sc[4]) ? sc[3] : -1; }
}

// In-block exclusive scan of deg[0..ns) (global) into ptr[row0 + r] = e0 + excl.
__device__ __forceinline__ void scan_degrees(const int32_t* deg, int ns, int32_t* ptr_out, int e0, int* part, int* total) {
    const int chunk = (ns + EX_BLOCK - 1) / EX_BLOCK;
    const int r0 = threadIdx.x * chunk, r1 = min(ns, r0 + chunk);
    int s = 0;
    for (int r = r0; r < r1; ++r) s += deg[r];
    part[threadIdx.x] = s;
    scan_partials(part, total);
    int run = e0 + part[threadIdx.x];
    for (int r = r0; r < r1; ++r) { ptr_out[r] = run; run += deg[r]; }
}

// Ordered compaction of the neighbours of v that are inside the subgraph, remapped to batch rows (out2: optional second copy -- the
// by-source CSR of a symmetric parent).  WT (weighted stores): the edge's weight wsrc[q] goes to wout / wout2 at the slot its endpoint goes to in out / out2.
// MASK: the neighbour id `excl` is left out (mask_excl; wave-uniform here, per group of eight lanes in group_fill_row) -- the predicate of the count walkers.
template <bool G, typename PT, bool WT = false, bool MASK = false>
__device__ __forceinline__ void wave_fill_row(const int64_t* ptr, const int32_t* idx, int64_t base, int v, const uint32_t* seen,
                                              const PT* pref, int row0, int32_t* out, int32_t* out2, int pos, int lane,
                                              const float* wsrc = nullptr, float* wout = nullptr, float* wout2 = nullptr, int excl = -1) {
    const int64_t a = ptr[base + v], b = ptr[base + v + 1];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t q = a; q < b; q += EX_WINFL * GM_WAVE) {
        int u[EX_WINFL];
#pragma unroll
        for (int k = 0; k < EX_WINFL; ++k) u[k] = q + k * GM_WAVE + lane < b ? idx[q + k * GM_WAVE + lane] : -1;
        float wv[EX_WINFL];
        if constexpr (WT) {
#pragma unroll
            for (int k = 0; k < EX_WINFL; ++k) wv[k] = q + k * GM_WAVE + lane < b ? wsrc[q + k * GM_WAVE + lane] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < EX_WINFL; ++k) {                     // in list order
            const int hit = u[k] >= 0 && (!MASK || u[k] != excl) && bit_test<G>(seen, u[k]);
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const int x = row0 + bit_rank<G, PT>(seen, pref, u[k]), p = pos + __popcll(m & lt); out[p] = x; if (out2) out2[p] = x;
                if constexpr (WT) { wout[p] = wv[k]; if (out2) wout2[p] = wv[k]; }
            }
            pos += __popcll(m);
        }
    }
}
// The same for one node per group of eight lanes (all lanes of the wave call it; a group without a node passes a == b)
template <bool G, typename PT, bool WT = false, bool MASK = false>
__device__ __forceinline__ void group_fill_row(const int64_t a, const int64_t b, const int32_t* idx, const uint32_t* seen, const PT* pref, int row0,
                                               int32_t* out, int32_t* out2, int pos, int grp, int gl,
                                               const float* wsrc = nullptr, float* wout = nullptr, float* wout2 = nullptr, int excl = -1) {
    const unsigned lt = (1u << gl) - 1u;
    for (int64_t q = a + gl; __any(q < b); q += EX_INFL * EX_GL) {
        int u[EX_INFL];
#pragma unroll
        for (int k = 0; k < EX_INFL; ++k) u[k] = q + k * EX_GL < b ? idx[q + k * EX_GL] : -1;
        float wv[EX_INFL];
        if constexpr (WT) {
#pragma unroll
            for (int k = 0; k < EX_INFL; ++k) wv[k] = q + k * EX_GL < b ? wsrc[q + k * EX_GL] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < EX_INFL; ++k) {                      // in list order: the k-th batch of eight neighbours after the (k-1)-th
            const int h = u[k] >= 0 && (!MASK || u[k] != excl) && bit_test<G>(seen, u[k]);
            const unsigned bm = (unsigned)(__ballot(h) >> (grp * EX_GL)) & 0xffu;
            if (h) {
                const int x = row0 + bit_rank<G, PT>(seen, pref, u[k]), p = pos + __popc(bm & lt); out[p] = x; if (out2) out2[p] = x;
                if constexpr (WT) { wout[p] = wv[k]; if (out2) wout2[p] = wv[k]; }
            }
            pos += __popc(bm);
        }
    }
}

// Phase B: write the batched CSR (by destination and by source), parents, feature rows, norm, centres.
// One launch may fill TWO batches (gm_extract_pair: the support and the query batch of a meta-batch): seeds [0, split) belong to o0, the rest to o1, each
// batch numbered from its own subgraph 0.  (The 288-subgraph support launch of a 32-task meta-batch was ~0.1 ms of one workgroup's latency chain on an otherwise
// empty GPU; as the head of the 2,592-workgroup joint launch it costs nothing.)
struct FillOut {
    const int32_t* sub_off; const int32_t* sub_eoff; int32_t* parent; int32_t* feat_row; float* norm;
    int32_t* indptr; int32_t* indices; int32_t* indptr_t; int32_t* indices_t; int32_t* centre;
};
// Weighted stores (WT): the store's edge weights in both orientations and the two batches' gm_batch::d_ew -- written at the slots where the fill writes
// indices / indices_t.  They ride in a LAST argument that only the weighted instantiations have, k_fill<G, P16, MASK, FillW>: with the empty pack the
// kernel takes the arguments it took before there were weights (even an empty struct there would move the hidden arguments a kernel reads blockDim from).
// MASK (GM_LINK_MASK_TARGET): the rows are filled without the target link, as k_nodes counted them.
struct FillW { const float* in_w; const float* out_w; float* ew0[2]; float* ew1[2]; };      // ew0 / ew1: d_ew of the batch o0 / o1 fills
template <bool G, bool P16 = false, bool MASK = false, typename... WArgs>
__global__ __launch_bounds__(EX_BLOCK) void k_fill(ExStore S, const gm_seed_t* seeds, int n_seeds, int link, int cap,
                                                   const int32_t* nodes_slab, const int32_t* degi_slab, const int32_t* dego_slab,
                                                   FillOut o0, FillOut o1, int split, int Wmax, uint32_t* gbits, const int32_t* order, WArgs... w_args) {
    constexpr bool WT = sizeof...(WArgs) != 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* seen = G ? gbits + (size_t)blockIdx.x * 2 * Wmax : lds;
    static_assert(!(G && P16), "16-bit prefix words live in LDS");
    typedef typename std::conditional<P16, uint16_t, uint32_t>::type PT;
    PT* pref = reinterpret_cast<PT*>(seen + Wmax);
    int* part = (int*)(G ? lds : lds + Wmax + (P16 ? (Wmax + 1) / 2 : Wmax));
    int* sc = part + EX_BLOCK;
    if ((int)blockIdx.x >= n_seeds) return;
    // workgroups start in blockIdx order: the subgraphs with the most edges first (host order, by the sizes the count pass brought), so that the last
    // of the ~2.5 rounds a 32-task meta-batch makes over the chip's workgroup slots is made of short ones
    const int seed = order ? order[blockIdx.x] : (int)blockIdx.x;
    const bool second = seed >= split;
    const int ls = second ? seed - split : seed, nl = second ? n_seeds - split : split;      // subgraph number inside its batch; the batch's subgraph count
    const int32_t* sub_off = second ? o1.sub_off : o0.sub_off; const int32_t* sub_eoff = second ? o1.sub_eoff : o0.sub_eoff;
    int32_t* parent = second ? o1.parent : o0.parent; int32_t* feat_row = second ? o1.feat_row : o0.feat_row; float* norm = second ? o1.norm : o0.norm;
    int32_t* indptr = second ? o1.indptr : o0.indptr; int32_t* indices = second ? o1.indices : o0.indices;
    int32_t* indptr_t = second ? o1.indptr_t : o0.indptr_t; int32_t* indices_t = second ? o1.indices_t : o0.indices_t; int32_t* centre = second ? o1.centre : o0.centre;
    const int g = seeds[seed].graph;
    const int64_t base = S.node_off[g];
    const int n = (int)(S.node_off[g + 1] - base);
    const int W = (n + 31) >> 5;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int row0 = sub_off[ls], ns = sub_off[ls + 1] - row0, e0 = sub_eoff[ls];
    const int32_t* nodes = nodes_slab + (int64_t)seed * cap;
    const int32_t* degi = degi_slab + (int64_t)seed * cap;
    const int32_t* dego = dego_slab + (int64_t)seed * cap;

    for (int w = tid; w < W; w += EX_BLOCK) wst<G>(&seen[w], 0u);
    __syncthreads();
    for (int r = tid; r < ns; r += EX_BLOCK) {
        const int v = nodes[r];
        bit_set(seen, v);
        parent[row0 + r] = v;
        feat_row[row0 + r] = (int32_t)(base + v);
        const int d = degi[r];
        norm[row0 + r] = 1.0f / sqrtf((float)(d > 1 ? d : 1));          // in_degrees().clamp(min=1) ** -0.5 (learner.py:29)
    }
    __syncthreads();
    bitmap_prefix<G, PT>(seen, pref, W, part, &sc[0]);
    scan_degrees(degi, ns, indptr + row0, e0, part, &sc[0]);
    scan_degrees(dego, ns, indptr_t + row0, e0, part, &sc[1]);
    if (ls == nl - 1 && tid == 0) { indptr[row0 + ns] = e0 + sc[0]; indptr_t[row0 + ns] = e0 + sc[1]; }
    __syncthreads();
    if (tid == 0) {
        const int nc = link ? 2 : 1;
        centre[ls * nc] = bit_rank<G, PT>(seen, pref, seeds[seed].i);
        if (link) centre[ls * nc + 1] = bit_rank<G, PT>(seen, pref, seeds[seed].j);
    }
    // walk_rows: eight rows per wave at a time, hub nodes by a whole wave afterwards.  A symmetric parent fills both orientations from the one walk.
    {
        const int grp = lane / EX_GL, gl = lane % EX_GL;
        int32_t* ind2 = S.sym ? indices_t : nullptr;
        [[maybe_unused]] int ci = -1, cj = -1;      // masked builds only: the two centres
        if constexpr (MASK) { ci = seeds[seed].i; cj = seeds[seed].j; }
        float* ew = nullptr; float* ew_t = nullptr;
        const float* in_w = nullptr; const float* out_w = nullptr;
        if constexpr (WT) {
            const FillW& fw = (w_args, ...);
            in_w = fw.in_w; out_w = fw.out_w; ew = second ? fw.ew1[0] : fw.ew0[0]; ew_t = second ? fw.ew1[1] : fw.ew0[1];
        }
        walk_rows<true>(S, base, nodes, ns, indptr + row0, indptr_t + row0, part, &sc[2], tid, wave, grp, gl,
            [&](bool, bool, int, int v, int64_t ia, int64_t ib, int64_t oa, int64_t ob, int pi, int po) {
                int excl = -1;
                if constexpr (MASK) excl = mask_excl(v, ci, cj);      // (v < 0: a group without a row, and ci, cj >= 0)
                group_fill_row<G, PT, WT, MASK>(ia, ib, S.in_idx, seen, pref, row0, indices, ind2, pi, grp, gl, in_w, ew, ew_t, excl);
                if (!S.sym) group_fill_row<G, PT, WT, MASK>(oa, ob, S.out_idx, seen, pref, row0, indices_t, nullptr, po, grp, gl, out_w, ew_t, nullptr, excl);
            },
            [&](int r, int v) {
                int excl = -1;
                if constexpr (MASK) excl = mask_excl(v, ci, cj);
                wave_fill_row<G, PT, WT, MASK>(S.in_ptr, S.in_idx, base, v, seen, pref, row0, indices, ind2, indptr[row0 + r], lane, in_w, ew, ew_t, excl);
                if (!S.sym) wave_fill_row<G, PT, WT, MASK>(S.out_ptr, S.out_idx, base, v, seen, pref, row0, indices_t, nullptr, indptr_t[row0 + r], lane, out_w, ew_t, nullptr, excl);
            });
    }
}
// Weighted batches: norm[r] = 1 / sqrt(d > 0 ? d : 1), d = the row's in-edge weights summed in edge order (k_fill knows only the count and wrote the
// unweighted norm; this launch replaces it).  All weights 1: d is the count, an exact integer, and the quotient below is k_fill's own expression.
__global__ void k_weighted_norm(const int32_t* indptr, const float* ew, int64_t rows, float* norm) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        float d = 0.f;
        for (int e = indptr[r], e1 = indptr[r + 1]; e < e1; ++e) d += ew[e];
        norm[r] = 1.0f / sqrtf(d > 0.f ? d : 1.0f);
    }
}

// per-edge tables: source norm (both orientations) and source feature row (forward orientation)
// Row gains of the aggregates (gm_batch::d_gain, zeroed): bit patterns of non-negative floats order as unsigned integers.
__global__ void k_gains(const int32_t* indptr, const int32_t* indices, const int32_t* indptr_t, const float* norm, int64_t rows, unsigned* gain) {
    float g0 = 0.f, g1 = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        // hub rows: norm <= 1, so the degree bounds the sum (their neighbours are mostly low-degree rows: within ~2x of it)
        const int e0 = indptr[i], e1 = indptr[i + 1];
        float s = (float)(e1 - e0);
        if (e1 - e0 <= 32) { s = 0.f; for (int e = e0; e < e1; ++e) s += norm[indices[e]]; }
        g0 = fmaxf(g0, s);
        g1 = fmaxf(g1, norm[i] * (float)(indptr_t[i + 1] - indptr_t[i]));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { g0 = fmaxf(g0, __shfl_xor(g0, o)); g1 = fmaxf(g1, __shfl_xor(g1, o)); }
    if ((threadIdx.x & 63) == 0) { if (g0 > 0.f) atomicMax(gain, __float_as_uint(g0)); if (g1 > 0.f) atomicMax(gain + 1, __float_as_uint(g1)); }
}

// (weighted batches, WArgs = {EdgeW}: the table carries the edge's weight too -- enorm[e] = w[e] * norm[u] is the aggregate's whole per-edge coefficient)
struct EdgeW { const float* ew; const float* ew_t; };      // gm_batch::d_ew
template <typename... WArgs>
__global__ void k_edge_tables(const int32_t* indices, const int32_t* indices_t, int64_t edges, const float* norm, const int32_t* feat_row,
                              float* enorm, float* enorm_t, int32_t* efeat, WArgs... w_args) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < edges; e += (int64_t)gridDim.x * blockDim.x) {
        const int u = indices[e], v = indices_t[e];
        if constexpr (sizeof...(WArgs) != 0) { const EdgeW& w = (w_args, ...); enorm[e] = w.ew[e] * norm[u]; enorm_t[e] = w.ew_t[e] * norm[v]; }
        else { enorm[e] = norm[u]; enorm_t[e] = norm[v]; }
        efeat[e] = feat_row[u];
    }
}
// ONE pass over the rows for everything the finalisation derives from the row bounds (round 6; four launches before): hub-row lists of both orientations (atomic append; the host orders them), the fused launch's per-row source table with its
// row / edge counts (gm_batch::d_fuse2 / d_fuse2_feat, unfused_rows / unfused_edges), and the keep-flag row scale gm_batch::d_norm_c with the sign bit set on
// every row (k_centre_rows clears it on the centre rows afterwards).  Hub rows: in-degree (o = 0) / out-degree (o = 1) above `thr`.
// Same pass: gm_batch::d_norm_src (the norm, sign bit set on the rows without an out-edge: nobody's source) with the count of the other rows as a third
// per-workgroup partial, and the all-zero entries of gm_batch::d_dq_tab (k_centre_rows writes the centre rows' afterwards).
// WT (weighted batches): the source table's w0 / w1 are ew[e] * norm[u], the products k_edge_tables<EdgeW> stores for the same edges.
struct RowW { const float* ew; };      // gm_batch::d_ew[0]
template <typename... WArgs>           // {}: the unweighted kernel, argument for argument; {RowW}: weighted batches
__global__ void k_row_tables(const int32_t* indptr, const int32_t* indices, const int32_t* indptr_t, int64_t rows, const float* norm, const int32_t* feat_row,
                             int4* f2, int4* f2_feat, unsigned long long* counts, int32_t* heavy0, int32_t* heavy1, int32_t* hcnt, int cap, int thr, float* norm_c,
                             int2* first0, int2* first1, int n_first, float* norm_src, int4* dq_tab, WArgs... w_args) {
    constexpr bool WT = sizeof...(WArgs) != 0;
    unsigned long long nr = 0, ne = 0, ns = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int p = indptr[r], d = indptr[r + 1] - p, dt = indptr_t[r + 1] - indptr_t[r];
        // [rows: cap][degrees: cap]; the first n_first (row, degree) pairs also go to the round trip's scratch (one download for everything the host waits for)
        // (one atomic per wave and orientation: the hub rows of a wave take consecutive slots; the lists are sorted on the host anyway)
        {
            const unsigned long long m0 = __ballot(d > thr), m1 = __ballot(dt > thr), below = (1ull << (threadIdx.x & 63)) - 1ull;
            if (m0) {
                const int lead = __ffsll((long long)m0) - 1;
                int base = ((int)(threadIdx.x & 63) == lead) ? atomicAdd(hcnt, __popcll(m0)) : 0;
                base = __shfl(base, lead, 64);
                if (d > thr) { const int k = base + __popcll(m0 & below); if (k < cap) { heavy0[k] = (int32_t)r; heavy0[cap + k] = d; } if (k < n_first) first0[k] = make_int2((int)r, d); }
            }
            if (m1) {
                const int lead = __ffsll((long long)m1) - 1;
                int base = ((int)(threadIdx.x & 63) == lead) ? atomicAdd(hcnt + 1, __popcll(m1)) : 0;
                base = __shfl(base, lead, 64);
                if (dt > thr) { const int k = base + __popcll(m1 & below); if (k < cap) { heavy1[k] = (int32_t)r; heavy1[cap + k] = dt; } if (k < n_first) first1[k] = make_int2((int)r, dt); }
            }
        }
        const float nrm = norm[r];
        norm_c[r] = __uint_as_float(__float_as_uint(nrm) | 0x80000000u);
        norm_src[r] = dt > 0 ? nrm : __uint_as_float(__float_as_uint(nrm) | 0x80000000u);
        if (dt > 0) ++ns;
        dq_tab[r] = make_int4(GM_FUSE_ZERO, GM_FUSE_ZERO, 0, 0);
        const int self = (int)r | GM_FUSE_SELF;
        int4 t = make_int4(self, self, __float_as_int(1.f), 0), tf = t;
        if (d == 0) { t = make_int4(GM_FUSE_ZERO, GM_FUSE_ZERO, __float_as_int(1.f), 0); tf = t; }
        else if (d <= GM_FUSE_MAXDEG) {
            const int u0 = indices[p], u1 = d >= 2 ? indices[p + 1] : u0;
            int w0, w1;
            if constexpr (WT) { const float* ew = (w_args, ...).ew; w0 = __float_as_int(ew[p] * norm[u0]); w1 = d >= 2 ? __float_as_int(ew[p + 1] * norm[u1]) : 0; }
            else { w0 = __float_as_int(norm[u0]); w1 = d >= 2 ? __float_as_int(norm[u1]) : 0; }
            t = make_int4(u0, u1, w0, w1); tf = make_int4(feat_row[u0], feat_row[u1], w0, w1);
        }
        if (d > GM_FUSE_MAXDEG) { ++nr; ne += (unsigned long long)d; }
        f2[r] = t; f2_feat[r] = tf;
    }
    // one pair of partials per WORKGROUP (wave shuffles, then the four wave partials through LDS): as atomics the two counters are a single contended
    // address each -- per thread 92k atomics took longer than the table itself, per wave the 16k of the 1.14 M-row batch still cost ~100 us
    __shared__ unsigned long long part[3][4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { nr += __shfl_down(nr, off, 64); ne += __shfl_down(ne, off, 64); ns += __shfl_down(ns, off, 64); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = nr; part[1][threadIdx.x >> 6] = ne; part[2][threadIdx.x >> 6] = ns; }
    __syncthreads();
    if (threadIdx.x == 0) {         // per-workgroup partials, summed by the host after the round trip (no same-address atomics at all: 2 x 2,048 of them were a third of this kernel)
        counts[3 * blockIdx.x] = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        counts[3 * blockIdx.x + 1] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
        counts[3 * blockIdx.x + 2] = part[2][0] + part[2][1] + part[2][2] + part[2][3];
    }
}
// distinct sources of the rows with more than maxdeg in-edges: mark, then count
__global__ void k_mark_sources(const int32_t* indptr, const int32_t* indices, int64_t rows, int maxdeg, uint32_t* bits) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int p = indptr[r], d = indptr[r + 1] - p;
        if (d > maxdeg) for (int e = p; e < p + d; ++e) { const int u = indices[e]; atomicOr(&bits[u >> 5], 1u << (u & 31)); }
    }
}
__global__ void k_count_bits(const uint32_t* bits, int64_t words, unsigned long long* out) {
    unsigned long long c = 0;
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) c += __popc(bits[w]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
int64_t gm_batch_unfused_sources(const gm_batch* b, hipStream_t s) {
    if (b->unfused_src >= 0) return b->unfused_src;
    const int64_t fallback = std::min<int64_t>(b->unfused_edges, b->rows);
    if (b->rows <= 0 || b->unfused_edges <= 0) return b->unfused_src = 0;
    const int64_t words = (b->rows + 31) / 32;
    uint32_t* bits = nullptr; unsigned long long* cnt = nullptr; unsigned long long h = 0;
    if (gm_alloc(&bits, (size_t)words, s) != GM_OK || gm_alloc(&cnt, 1, s) != GM_OK) { gm_dev_free(bits, s); return fallback; }
    bool ok = hipMemsetAsync(bits, 0, 4 * (size_t)words, s) == hipSuccess && hipMemsetAsync(cnt, 0, 8, s) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_mark_sources, dim3((int)std::min<int64_t>(2048, (b->rows + 255) / 256)), dim3(256), 0, s, b->d_indptr, b->d_indices, (int64_t)b->rows, GM_FUSE_MAXDEG, bits);
        hipLaunchKernelGGL(k_count_bits, dim3((int)std::min<int64_t>(512, (words + 255) / 256)), dim3(256), 0, s, bits, words, cnt);
        ok = hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    gm_dev_free(bits, s); gm_dev_free(cnt, s);
    return ok ? (b->unfused_src = (int64_t)h) : fallback;
}
// Ordered compaction of the rows with lo <= in-degree <= hi (the window rows of a partial aggregate launch) and, with `flag`, its sign bit clear (the observable ones
// among them: gm_batch::obs): per-block counts, a one-block scan of the counts, then every block writes its rows at its offset (ballot ranks: ascending row ids).
// total (with cap): the scan leaves the list's length there, for the launches that learn it on the device (never above the cap the list was allocated for).
#define MID_BLOCK 1024
__device__ __forceinline__ bool mid_row(const int32_t* indptr, const float* flag, int64_t r, int64_t rows, int lo, int hi) {
    if (r >= rows) return false;
    const int d = indptr[r + 1] - indptr[r];
    return d >= lo && d <= hi && !(flag && (__float_as_uint(flag[r]) >> 31));
}
__global__ __launch_bounds__(MID_BLOCK) void k_mid_count(const int32_t* indptr, const float* flag, int64_t rows, int lo, int hi, int32_t* bcnt) {
    __shared__ int wsum[MID_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * MID_BLOCK + threadIdx.x;
    const unsigned long long m = __ballot(mid_row(indptr, flag, r, rows, lo, hi));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < MID_BLOCK / 64; ++k) t += wsum[k]; bcnt[blockIdx.x] = t; }
}
__global__ __launch_bounds__(1024) void k_mid_scan(int32_t* bcnt, int nb, int32_t* total, int cap) {      // exclusive scan in place, one block
    __shared__ int part[1024];
    const int per = (nb + 1023) / 1024, a = threadIdx.x * per, b = min(nb, a + per);
    int t = 0;
    for (int k = a; k < b; ++k) t += bcnt[k];
    part[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) { int run = 0; for (int k = 0; k < 1024; ++k) { const int v = part[k]; part[k] = run; run += v; } }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int k = a; k < b; ++k) { const int v = bcnt[k]; bcnt[k] = run; run += v; }
    if (total && threadIdx.x == 1023) *total = min(run, cap);      // (the last thread's run ends at the sum of every count)
}
__global__ __launch_bounds__(MID_BLOCK) void k_mid_scatter(const int32_t* indptr, const float* flag, int64_t rows, int lo, int hi, const int32_t* boff, int32_t* list, int cap) {
    __shared__ int wsum[MID_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * MID_BLOCK + threadIdx.x;
    const bool f = mid_row(indptr, flag, r, rows, lo, hi);
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int base = boff[blockIdx.x];
    for (int k = 0; k < wv; ++k) base += wsum[k];
    const int at = base + __popcll(m & ((1ull << lane) - 1ull));
    if (f && at < cap) list[at] = (int32_t)r;
}
// centre rows, their norms and in-degrees (row-sparse backward tables)
// (norm_c != NULL: also clears the keep-flag scale's sign bit on the centre rows -- after k_row_tables set it on every row)
__global__ void k_centre_rows(const int32_t* sub_off, const int32_t* centre, int nc, int n_c, const int32_t* indptr, const float* norm,
                              int32_t* crow, float* cnorm, int32_t* cdeg, float* norm_c, int32_t* centre_copy, int4* dq_tab) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_c) return;
    const int row = sub_off[k / nc] + centre[k];
    centre_copy[k] = centre[k];
    crow[k] = row; cnorm[k] = norm[row]; cdeg[k] = indptr[row + 1] - indptr[row];
    if (norm_c) norm_c[row] = __uint_as_float(__float_as_uint(norm[row]) & 0x7fffffffu);
    if (dq_tab) dq_tab[row] = make_int4(row | GM_FUSE_SELF, GM_FUSE_ZERO, __float_as_int(1.f), 0);      // (two centres on one row write the same entry)
}
struct CentreW { const float* ew; float* e_coef; };      // weighted batches: gm_batch::d_ew[0] -> gm_batch::d_e1_coef = weight x source norm of every centre in-edge
template <typename... WArgs>                              // {}: the unweighted kernel, argument for argument; {CentreW}: weighted batches
__global__ void k_centre_edges(const int32_t* crow, const int32_t* eoff, int n_c, const int32_t* indptr, const int32_t* indices,
                               const float* norm, int32_t* e_row, int32_t* e_par, float* e_norm, WArgs... w_args) {
    const int k = blockIdx.x;
    if (k >= n_c) return;
    const int p0 = indptr[crow[k]], n = eoff[k + 1] - eoff[k], o = eoff[k];
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int u = indices[p0 + j]; e_row[o + j] = u; e_par[o + j] = k; e_norm[o + j] = norm[u];
        if constexpr (sizeof...(WArgs) != 0) { const CentreW& cw = (w_args, ...); cw.e_coef[o + j] = cw.ew[p0 + j] * norm[u]; }
    }
}
// GM_DEAD_ROWS=2 tables (gm_batch::d_ect / d_norm_e1).  First pass: every row's norm with the sign bit set, and every by-source edge's row of T -- its destination
// where that is a centre (sign bit of norm_c clear), else a row of the zero block behind T.  Second pass, over the centres' in-edges: the sign bit cleared on
// their source rows; the first clear of a row counts it.
__global__ void k_e1_tables(const int32_t* indices_t, int64_t edges, const float* norm, const float* norm_c, int64_t rows, int32_t* ect, float* norm_e1, int32_t* n_rows) {
    const int64_t n = edges > rows ? edges : rows;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_rows = 0;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        if (k < rows) norm_e1[k] = __uint_as_float(__float_as_uint(norm[k]) | 0x80000000u);
        if (k < edges) { const int v = indices_t[k]; ect[k] = (__float_as_uint(norm_c[v]) >> 31) ? (int32_t)(rows + (k & (GM_ZERO_ROWS - 1))) : v; }
    }
}
__global__ void k_e1_rows(const int32_t* e_row, int n_e1, float* norm_e1, int32_t* n_rows) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_e1) return;
    const unsigned old = atomicAnd(reinterpret_cast<unsigned*>(norm_e1) + e_row[k], 0x7fffffffu);
    if (old >> 31) atomicAdd(n_rows, 1);
}
int64_t gm_batch_e1_rows(const gm_batch* b, hipStream_t s) {
    if (b->n_e1_rows >= 0) return b->n_e1_rows;
    const int64_t fallback = std::min<int64_t>(b->n_e1, b->rows);
    if (!b->d_n_e1_rows) return fallback;
    int32_t h = 0;
    if (hipMemcpyAsync(&h, b->d_n_e1_rows, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return fallback; }
    return b->n_e1_rows = h;
}
// by-source edges of the rows d_norm_e1 keeps (what the keep_signed aggregate walks): counted at first use, like gm_batch_unfused_sources
__global__ void k_e1_kept_edges(const int32_t* indptr_t, const float* norm_e1, int64_t rows, unsigned long long* out) {
    unsigned long long c = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x)
        if (!(__float_as_uint(norm_e1[r]) >> 31)) c += (unsigned long long)(indptr_t[r + 1] - indptr_t[r]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
int64_t gm_batch_e1_edges(const gm_batch* b, hipStream_t s) {
    if (b->n_e1_edges >= 0) return b->n_e1_edges;
    const int64_t fallback = b->edges;
    if (!b->d_norm_e1 || !b->d_indptr_t || b->rows <= 0) return fallback;
    unsigned long long* cnt = nullptr; unsigned long long h = 0;
    if (gm_alloc(&cnt, 1, s) != GM_OK) return fallback;
    bool ok = hipMemsetAsync(cnt, 0, 8, s) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_e1_kept_edges, dim3((int)std::min<int64_t>(512, (b->rows + 255) / 256)), dim3(256), 0, s, b->d_indptr_t, b->d_norm_e1, (int64_t)b->rows, cnt);
        ok = hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    if (!ok) (void)hipGetLastError();
    gm_dev_free(cnt, s);
    return ok ? (b->n_e1_edges = (int64_t)h) : fallback;
}
// GM_DEAD_ROWS=3 tables (gm_batch::d_fwd_tab / d_fwd_tab_feat / d_obs), after k_e1_rows: the source tables and the keep flags of the passes nobody differentiates.
// A row is observable in the last layer where it is a centre (sign bit of norm_c clear), in the layer below where it is the source of an in-edge of a centre
// (sign bit of norm_e1 clear): there it keeps d_fuse2's (d_fuse2_feat's) entry and the flag +1, everywhere else it reads the zero row and carries -1
__global__ void k_fwd_tables(const int4* f2, const int4* f2_feat, const float* norm_c, const float* norm_e1, int64_t rows, int4* tab_c, int4* tab_e1, int4* tab_e1_feat,
                             float* obs_c, float* obs_e1) {
    auto pick = [](const bool on, const int4 t) { return make_int4(on ? t.x : GM_FUSE_ZERO, on ? t.y : GM_FUSE_ZERO, on ? t.z : 0, on ? t.w : 0); };
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const bool c = !(__float_as_uint(norm_c[r]) >> 31), e = !(__float_as_uint(norm_e1[r]) >> 31);
        const int4 t = f2[r], tf = f2_feat[r];
        tab_c[r] = pick(c, t); tab_e1[r] = pick(e, t); tab_e1_feat[r] = pick(e, tf);
        obs_c[r] = c ? 1.f : -1.f; obs_e1[r] = e ? 1.f : -1.f;
    }
}
// GM_DEAD_TILES flags (gm_batch::d_tile_live): one block per GEMM row tile {set, row0, nrows <= GM_GEMM_BM}; live_c / live_e1[tile] = 1 where some row of the tile has
// the sign bit of norm_c / norm_e1 clear, else 0
__global__ __launch_bounds__(GM_GEMM_BM) void k_tile_live(const int32_t* tiles, int n_tiles, const float* norm_c, const float* norm_e1, int32_t* live_c, int32_t* live_e1) {
    const int t = blockIdx.x;
    if (t >= n_tiles) return;
    const int row0 = tiles[3 * t + 1], nrows = tiles[3 * t + 2], r = threadIdx.x;
    const bool in = r < nrows;
    const int c = in && !(__float_as_uint(norm_c[(int64_t)row0 + r]) >> 31), e = in && !(__float_as_uint(norm_e1[(int64_t)row0 + r]) >> 31);
    const int any_c = __syncthreads_or(c), any_e = __syncthreads_or(e);
    if (r == 0) { live_c[t] = any_c ? 1 : 0; live_e1[t] = any_e ? 1 : 0; }
}
// GM_PACK_ROWS tables (gm_batch::pack): one block per set walks the set's rows in ascending order and appends every row with the sign bit of `keep` clear to the set's
// region [base[t], base[t + 1]) of the packed arrays: its row id, |keep|, and its entries of up to two per-row tables.  cnt[t]: the rows appended (never more than the
// region holds: base comes from the host's bounds of the same counts)
#define PACK_BLOCK 1024
__global__ __launch_bounds__(PACK_BLOCK) void k_pack_rows(const int32_t* set_row_off, const int32_t* base, const float* keep, const int4* src0, const int4* src1,
                                                          int32_t* rowid, float* scale, int4* dst0, int4* dst1, int32_t* cnt) {
    __shared__ int wsum[PACK_BLOCK / 64];
    const int t = blockIdx.x, r0 = set_row_off[t], r1 = set_row_off[t + 1], o0 = base[t], room = base[t + 1] - o0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int done = 0;
    for (int rb = r0; rb < r1; rb += PACK_BLOCK) {
        const int r = rb + threadIdx.x;
        const float kv = r < r1 ? keep[r] : -1.f;
        const bool on = r < r1 && !(__float_as_uint(kv) >> 31);
        const unsigned long long m = __ballot(on);
        if (lane == 0) wsum[w] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < PACK_BLOCK / 64; ++k) { const int c = wsum[k]; before += k < w ? c : 0; all += c; }
        const int at = done + before + __popcll(m & ((1ull << lane) - 1ull));
        if (on && at < room) {
            rowid[o0 + at] = r; scale[o0 + at] = kv;
            if (src0) dst0[o0 + at] = src0[r];
            if (src1) dst1[o0 + at] = src1[r];
        }
        done += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[t] = done < room ? done : room;
}
// ... and the packed tile table {set, offset, nrows <= GM_GEMM_BM} over those counts, sets in order, with the number of tiles in *count (one block)
__global__ __launch_bounds__(64) void k_pack_tiles(const int32_t* cnt, const int32_t* base, int sets, int cap_tiles, int32_t* tiles, int32_t* count) {
    __shared__ int first;
    if (threadIdx.x == 0) first = 0;
    __syncthreads();
    for (int t = 0; t < sets; ++t) {
        const int n = cnt[t], nt = (n + GM_GEMM_BM - 1) / GM_GEMM_BM, f = first;
        for (int j = threadIdx.x; j < nt; j += blockDim.x)
            if (f + j < cap_tiles) { int32_t* q = tiles + 3 * (int64_t)(f + j); q[0] = t; q[1] = base[t] + j * GM_GEMM_BM; q[2] = min(GM_GEMM_BM, n - j * GM_GEMM_BM); }
        __syncthreads();
        if (threadIdx.x == 0) first = min(cap_tiles, f + nt);
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = first;
}
// what the partial aggregate launch over flag vector `obs` touches: rows of more than maxdeg in-edges with a positive flag and their in-edges (out[0], out[1]); their
// sources marked in `bits` (k_count_bits counts them)
__global__ void k_fwd_count(const int32_t* indptr, const int32_t* indices, const float* obs, int64_t rows, int maxdeg, uint32_t* bits, unsigned long long* out) {
    unsigned long long nr = 0, ne = 0;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int p = indptr[r], d = indptr[r + 1] - p;
        if (d <= maxdeg || (__float_as_uint(obs[r]) >> 31)) continue;
        ++nr; ne += (unsigned long long)d;
        for (int e = p; e < p + d; ++e) { const int u = indices[e]; atomicOr(&bits[u >> 5], 1u << (u & 31)); }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { nr += __shfl_down(nr, off, 64); ne += __shfl_down(ne, off, 64); }
    if ((threadIdx.x & 63) == 0 && nr) { atomicAdd(out, nr); atomicAdd(out + 1, ne); }
}
int gm_batch_fwd_counts(const gm_batch* b, int which, hipStream_t s, int64_t* out) {
    GM_REQUIRE(b && out && (which == 0 || which == 1), GM_EINVAL, "batch_fwd_counts: bad arguments");
    int64_t* have = b->fwd_cnt[which];
    if (have[0] < 0) {
        GM_REQUIRE(b->d_obs[which] && b->rows > 0, GM_EINVAL, "batch_fwd_counts: the batch carries no forward-only tables");
        const int64_t words = (b->rows + 31) / 32;
        uint32_t* bits = nullptr; unsigned long long* cnt = nullptr; unsigned long long h[3] = {0, 0, 0};
        int rc = gm_alloc(&bits, (size_t)words, s);
        if (rc == GM_OK) rc = gm_alloc(&cnt, 3, s);
        bool ok = rc == GM_OK && hipMemsetAsync(bits, 0, 4 * (size_t)words, s) == hipSuccess && hipMemsetAsync(cnt, 0, 24, s) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(k_fwd_count, dim3((int)std::min<int64_t>(2048, (b->rows + 255) / 256)), dim3(256), 0, s, b->d_indptr, b->d_indices, b->d_obs[which], (int64_t)b->rows,
                               GM_FUSE_MAXDEG, bits, cnt);
            hipLaunchKernelGGL(k_count_bits, dim3((int)std::min<int64_t>(512, (words + 255) / 256)), dim3(256), 0, s, bits, words, cnt + 2);
            ok = hipMemcpyAsync(h, cnt, 24, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        }
        if (bits) gm_dev_free(bits, s);
        if (cnt) gm_dev_free(cnt, s);
        if (!ok) { (void)hipGetLastError(); gm_set_error("batch_fwd_counts: counting failed"); return GM_EHIP; }
        have[1] = (int64_t)h[1]; have[2] = (int64_t)h[2]; have[0] = (int64_t)h[0];
    }
    out[0] = have[0]; out[1] = have[1]; out[2] = have[2];
    return GM_OK;
}
__global__ void k_copy_add(int32_t* dst, const int32_t* src, int64_t n, int32_t add) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) dst[k] = src[k] + add;
}
__global__ void k_gather_rows(const float* feat, int64_t ld, const int32_t* feat_row, float* out, int64_t rows, int F) {
    const int64_t total = rows * F;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = k / F; const int f = (int)(k - r * F);
        out[k] = feat[(int64_t)feat_row[r] * ld + f];
    }
}

// ---- hop-distance node labels (gm_set_hop_labels, include/gmeta_hip.h): the labelling step of local-subgraph methods, beyond the reference
// One workgroup per (subgraph, centre): level-synchronous BFS from the centre along the in-edges of the batch's own induced CSR, at most D levels.
// label = distance where <= D, D + 1 for everything farther or unreachable (every row starts there).  A wave takes a frontier row, its lanes the
// row's in-edges; the writers racing for a row within a level all write that level.  The distance bytes live in LDS while the subgraph fits
// (sample_nodes + 2 rows: 1,002 by default), in the output array itself above that (workgroup-scope visibility: volatile accesses + the barrier).
#define GM_HOP_LDS_ROWS 2048
#define GM_HOP_BLOCK 256
template <bool LDS>
__device__ __forceinline__ void hop_bfs(int8_t* dist, int64_t stride, int n, int root, int r0, const int32_t* indptr, const int32_t* indices, int D) {
    auto get = [&](int v) -> int { return LDS ? (int)dist[v] : (int)((volatile int8_t*)dist)[(int64_t)v * stride]; };
    auto put = [&](int v, int d) { if (LDS) dist[v] = (int8_t)d; else ((volatile int8_t*)dist)[(int64_t)v * stride] = (int8_t)d; };
    const int far = D + 1, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int v = threadIdx.x; v < n; v += GM_HOP_BLOCK) put(v, v == root ? 0 : far);
    __syncthreads();
    for (int level = 1; level <= D; ++level) {
        for (int v = wave; v < n; v += GM_HOP_BLOCK / 64) {
            if (get(v) != level - 1) continue;                        // (wave-uniform)
            const int e1 = indptr[r0 + v + 1];
            for (int e = indptr[r0 + v] + lane; e < e1; e += 64) {
                const int u = indices[e] - r0;
                if ((unsigned)u < (unsigned)n && get(u) == far) put(u, level);
            }
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(GM_HOP_BLOCK) void k_hop_labels(const int32_t* sub_off, const int32_t* centre, int nc, const int32_t* indptr, const int32_t* indices, int D,
                                                             int8_t* hop) {
    __shared__ int8_t dist_s[GM_HOP_LDS_ROWS];
    const int k = blockIdx.x / nc, c = blockIdx.x - k * nc;
    const int r0 = sub_off[k], n = sub_off[k + 1] - r0, root = centre[k * nc + c];
    int8_t* out = hop + (int64_t)r0 * nc + c;                         // row v of the subgraph: out[v * nc]
    if (n <= GM_HOP_LDS_ROWS) {
        hop_bfs<true>(dist_s, 1, n, root, r0, indptr, indices, D);
        for (int v = threadIdx.x; v < n; v += GM_HOP_BLOCK) out[(int64_t)v * nc] = dist_s[v];
    } else hop_bfs<false>(out, nc, n, root, r0, indptr, indices, D);
}
// The labelled feature table of a batch: row r = [the store's feature row | one one-hot block of Lw columns per centre | zeros up to ldo] (ldo % 4 == 0),
// 16-byte loads from the store where its leading dimension allows, 16-byte stores; the same pass writes the identity row table the layer-1 readers
// address the table through.
__global__ void k_label_features(const float* feat, int64_t ld, int F0, const int32_t* store_row, const int8_t* hop, int nc, int Lw, float* out, int ldo, int64_t rows,
                                 int32_t* ident) {
    const int groups = ldo >> 2;
    const bool vec = (ld & 3) == 0;
    const int64_t total = rows * groups;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = k / groups; const int g = (int)(k - r * groups), c0 = 4 * g;
        const float* x = feat + (int64_t)store_row[r] * ld;
        float4 v;
        if (vec && c0 + 4 <= F0) v = *reinterpret_cast<const float4*>(x + c0);
        else {
            float t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q;
                if (c < F0) t[q] = x[c];
                else { const int j = c - F0, blk = j / Lw; t[q] = (blk < nc && (int)hop[r * nc + blk] == j - blk * Lw) ? 1.f : 0.f; }
            }
            v = make_float4(t[0], t[1], t[2], t[3]);
        }
        *reinterpret_cast<float4*>(out + r * (int64_t)ldo + c0) = v;
        if (g == 0) ident[r] = (int32_t)r;
    }
}

// ------------------------------------------------------------------------------------------ host
// workgroups of 256 threads over n items, `cap` at most (the kernels stride over the rest)
static inline int grid_for(int64_t n, int cap) { return (int)std::min<int64_t>(cap, (n + 255) / 256); }
// a new batch reads the store's feature table; with D > 0 the finalisation replaces it by the batch's own labelled table (label_batch)
static void batch_features(gm_batch* b, int D) {
    b->feat = b->store->d_feat; b->feat_ld = b->store->feat_ld; b->feat_dim = b->store->feat_dim; b->feat_rows = b->store->total_nodes; b->hop_D = D;
}
// Finalisation of a labelled batch, before the edge / row tables are derived (they then come out with identity feature rows): labels, the batch's
// feature table, and the row tables swapped -- d_store_row keeps the store rows (GM_F_FEAT_ROW)
static int label_batch(gm_batch* b, hipStream_t s) {
    const int D = b->hop_D, nc = b->centres, Fd = gm_hop_feat_dim(b->store, nc, D), ldo = gm_pad_feat(Fd);
    float* tab = nullptr; int32_t* ident = nullptr;
    GM_TRY(gm_balloc(b, &b->d_hop, (size_t)b->rows * nc, s)); GM_TRY(gm_balloc(b, &tab, (size_t)b->rows * ldo, s)); GM_TRY(gm_balloc(b, &ident, (size_t)b->rows, s));
    if (b->rows > 0) {
        hipLaunchKernelGGL(k_hop_labels, dim3(b->subs * nc), dim3(GM_HOP_BLOCK), 0, s, b->d_sub_off, b->d_centre, nc, b->d_indptr, b->d_indices, D, b->d_hop);
        hipLaunchKernelGGL(k_label_features, dim3(grid_for(b->rows * (ldo / 4), 4096)), dim3(256), 0, s, b->store->d_feat, (int64_t)b->store->feat_ld, b->store->feat_dim, b->d_feat_row, b->d_hop, nc, D + 2, tab, ldo, (int64_t)b->rows, ident);
        GM_HIP(hipGetLastError());
    }
    b->d_store_row = b->d_feat_row; b->d_feat_row = ident;
    b->feat = tab; b->feat_ld = ldo; b->feat_dim = Fd; b->feat_rows = b->rows;
    return GM_OK;
}

// Row gains of the two aggregates (gm_bound.h): only the opt-in two-piece kernels read them, so they are computed at first use (on `s`,
// ordered behind the batch's build) instead of in every batch finalisation (k_gains was the longest finalisation kernel: 0.2 ms on the 1.14 M-row
// query batch).  At least 1: an isolated row still passes its own magnitude on wherever a kernel adds a self term.
int gm_batch_gains(const gm_batch* cb, hipStream_t s) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    gm_batch* b = const_cast<gm_batch*>(cb);
    if (b->d_gain) return GM_OK;
    float* g = nullptr;
    GM_TRY(gm_balloc(b, &g, (size_t)2, b->stream));                                        // (the batch's slabs: freed with it, on its own stream)
    GM_TRY(gm_batch_wait_build(b, s));
    GM_HIP(hipMemsetD32Async((hipDeviceptr_t)g, 0x3f800000, 2, s));                        // 1.0f, 1.0f
    if (b->rows > 0) {
        hipLaunchKernelGGL(k_gains, dim3(grid_for(b->rows, 2048)), dim3(256), 0, s, b->d_indptr, b->d_indices, b->d_indptr_t, b->d_norm, (int64_t)b->rows, reinterpret_cast<unsigned*>(g));
        GM_HIP(hipGetLastError());
    }
    b->d_gain = g;
    gm_batch_mark_use(b, s);
    return GM_OK;
}

// Launch tables and derived per-batch tables.  ONE host round trip: the kernels whose results the host needs (hub-row lists, the fused launch's
// row / edge counts, the centres' in-degrees) are launched back to back, their results come back in one batch of copies into pinned memory,
// and everything the host derives from them goes up through pinned staging without waiting (gm_stager).
#define GM_HEAVY_FIRST 8192     // hub rows per orientation fetched with the first round trip (more: one more round trip)
// Hub rows come back in atomic-append order; the schedules want them ascending (and the build deterministic).  The rows are distinct ids below
// `rows`: an LSD radix sort, 11 bits a pass (two passes up to 4 M rows), carries the degrees along -- std::sort on the pairs cost 0.2 ms per
// orientation of the 1.14 M-row query batch, on the host, between the build's kernels.
static void sort_rows_with_degrees(std::vector<int32_t>& row, std::vector<int32_t>& deg, int64_t rows) {
    const size_t n = row.size();
    if (n < 2) return;
    std::vector<int32_t> row2(n), deg2(n);
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < rows) ++bits;
    int32_t* r0 = row.data(); int32_t* d0 = deg.data(); int32_t* r1 = row2.data(); int32_t* d1 = deg2.data();
    for (int shift = 0; shift < bits; shift += 11) {
        uint32_t cnt[2049] = {};
        for (size_t k = 0; k < n; ++k) ++cnt[(((uint32_t)r0[k] >> shift) & 2047u) + 1];
        for (int k = 0; k < 2048; ++k) cnt[k + 1] += cnt[k];
        for (size_t k = 0; k < n; ++k) { const uint32_t at = cnt[((uint32_t)r0[k] >> shift) & 2047u]++; r1[at] = r0[k]; d1[at] = d0[k]; }
        std::swap(r0, r1); std::swap(d0, d1);
    }
    if (r0 != row.data()) { row.swap(row2); deg.swap(deg2); }
}
// Scratch of the finalisation's round trip: ONE allocation, ONE memset (its first 32 bytes), ONE download.  Offsets in ints, the same on the device and in
// the downloaded copy: [4,6) hub-row counts | [8, 8 + n_c) centre in-degrees | n_c local centre ids | 2 x `first` (row, degree) pairs of the hub lists |
// k_row_tables' per-workgroup {rows, edges, rows with an out-edge} partials (u64 triples)
struct FinalScratch {
    int first = 0, rt_blocks = 1;      // hub rows per orientation the first fetch carries; k_row_tables' grid (512 .. 8,192 workgroups: the same 91 us on the query batch)
    size_t o_cnt = 4, o_cdeg = 8, o_centre = 0, o_first = 0, o_part = 0, ints = 0;
    void plan(int64_t rows, int n_c, int cap) {
        first = std::min(cap, GM_HEAVY_FIRST); rt_blocks = std::max(1, grid_for(rows, 2048));
        o_centre = o_cdeg + (size_t)n_c; o_first = (o_centre + n_c + 1) / 2 * 2; o_part = o_first + 4 * (size_t)first; ints = o_part + 6 * (size_t)rt_blocks;
    }
    template <class I> I* pairs(I* base, int o) const { return base + o_first + 2 * (size_t)first * o; }      // hub list of orientation o
};
// The finalisation in two halves around its host round trip, so that a caller that builds TWO batches (gm_extract_pair) queues both batches' kernels,
// waits once, and derives both batches' host-side tables while nothing is left to wait for.
struct FinalizeCtx {
    int cap = 0; FinalScratch lay;
    int32_t* scratch = nullptr; hipStream_t s = nullptr;         // device side of the round trip (finalize_launch); released by finalize_finish or on the way out
    const int32_t* h_scr = nullptr;                              // its downloaded copy
    FinalizeCtx() = default;
    FinalizeCtx(const FinalizeCtx&) = delete;
    FinalizeCtx& operator=(const FinalizeCtx&) = delete;
    ~FinalizeCtx() { if (scratch) gm_dev_free(scratch, s); }
};
// several small host tables into ONE region of the batch's slabs (gm_batch_destroy releases nothing else) with ONE copy through pinned staging; each part
// starts on a 256-byte boundary.  (One hipMemcpyAsync per table before: ~20 of the ~43 copies of a meta-batch build.)
struct TabPart { int32_t** d; const std::vector<int32_t>* v; };
static int upload_tables(gm_batch* b, gm_stager& sg, hipStream_t s, std::initializer_list<TabPart> parts) {
    auto pad = [](size_t n) { return (std::max<size_t>(n, 1) + 63) / 64 * 64; };
    size_t tot = 0;
    for (const TabPart& p : parts) tot += pad(p.v->size());
    int32_t* base = nullptr;
    GM_TRY(gm_balloc(b, &base, tot, s));
    std::vector<int32_t> h(tot, 0);
    size_t o = 0;
    for (const TabPart& p : parts) { std::copy(p.v->begin(), p.v->end(), h.begin() + o); *p.d = base + o; o += pad(p.v->size()); }
    return sg.upload(base, h);
}
// the {set, start, length} spans that cut every set's range [off[t], off[t + 1]) into pieces of `step`: GEMM row tiles, weight-gradient chunks (neither
// straddles two sets: each set has its own fast weights); set_first [sets + 1]: the first span of every set
static std::vector<int32_t> set_spans(const std::vector<int32_t>& off, int step, std::vector<int32_t>* set_first = nullptr) {
    std::vector<int32_t> v;
    if (set_first) set_first->assign(1, 0);
    for (int t = 0; t + 1 < (int)off.size(); ++t) {
        for (int r = off[t]; r < off[t + 1]; r += step) { v.push_back(t); v.push_back(r); v.push_back(std::min(step, off[t + 1] - r)); }
        if (set_first) set_first->push_back((int32_t)(v.size() / 3));
    }
    return v;
}
// Launch tables derived from the set layout (weight-gradient chunks are sized by gm_wgrad_chunk_rows), then the device side of the round trip
static int finalize_launch(gm_batch* b, hipStream_t s, gm_stager& sg, FinalizeCtx& fc) {
    gm_phase_timer tm("finalize-launch");
    std::vector<int32_t> sub_set(b->subs), set_chunk_off;
    for (int t = 0; t < b->sets; ++t)
        for (int k = b->h_set_sub_off[t]; k < b->h_set_sub_off[t + 1]; ++k) sub_set[k] = t;
    const std::vector<int32_t> tiles = set_spans(b->h_set_row_off, GM_GEMM_BM), chunks = set_spans(b->h_set_row_off, gm_wgrad_chunk_rows(b->h_set_row_off), &set_chunk_off);
    b->n_tiles = (int32_t)(tiles.size() / 3); b->n_chunks = (int32_t)(chunks.size() / 3);
    GM_TRY(upload_tables(b, sg, s, {{&b->d_sub_set, &sub_set}, {&b->d_tiles, &tiles}, {&b->d_chunks, &chunks}, {&b->d_set_chunk_off, &set_chunk_off}}));
    tm.lap("tables");
    if (b->hop_D > 0) GM_TRY(label_batch(b, s)); else b->d_store_row = b->d_feat_row;
    // ---- device side, nothing here waits for the host: hub-row lists of both orientations, per-edge tables, the fused launch's row table +
    // counts, centre rows with their in-degrees
    b->heavy_deg = gm_heavy_deg_for(b->rows, b->edges);
    const int cap = fc.cap = (int)(b->edges / b->heavy_deg + 1);
    const int nc = b->centres; b->n_c = b->subs * nc;
    FinalScratch& lay = fc.lay;
    lay.plan(b->rows, b->n_c, cap);
    GM_TRY(gm_alloc(&fc.scratch, lay.ints, s));
    fc.s = s;
    int32_t* const scr = fc.scratch;
    GM_HIP(hipMemsetAsync(scr, 0, 32, s));
    for (int o = 0; o < 2; ++o) GM_TRY(gm_balloc(b, &b->d_heavy[o], 2 * (size_t)cap, s));
    // the weighted kernel of every pair takes the unweighted one's arguments and its weights (w: none on unweighted batches)
    if (b->edges > 0) {
        GM_TRY(gm_balloc(b, &b->d_enorm[0], (size_t)b->edges, s)); GM_TRY(gm_balloc(b, &b->d_enorm[1], (size_t)b->edges, s)); GM_TRY(gm_balloc(b, &b->d_efeat, (size_t)b->edges, s));
        auto edge_tables = [&](auto kern, auto... w) {
            hipLaunchKernelGGL(kern, dim3(grid_for(b->edges, 4096)), dim3(256), 0, s, b->d_indices, b->d_indices_t, (int64_t)b->edges, b->d_norm, b->d_feat_row, b->d_enorm[0], b->d_enorm[1], b->d_efeat, w...);
        };
        if (b->weighted) edge_tables(k_edge_tables<EdgeW>, EdgeW{b->d_ew[0], b->d_ew[1]}); else edge_tables(k_edge_tables<>);
    }
    GM_TRY(gm_balloc(b, &b->d_norm_c, b->rows, s)); GM_TRY(gm_balloc(b, &b->d_norm_src, b->rows, s));
    if (b->rows > 0) {
        int4 *f0 = nullptr, *ff = nullptr, *fd = nullptr;
        GM_TRY(gm_balloc(b, &f0, (size_t)b->rows, s)); GM_TRY(gm_balloc(b, &ff, (size_t)b->rows, s)); GM_TRY(gm_balloc(b, &fd, (size_t)b->rows, s));
        b->d_fuse2 = f0; b->d_fuse2_feat = ff; b->d_dq_tab = fd;
        auto row_tables = [&](auto kern, auto... w) {
            hipLaunchKernelGGL(kern, dim3(lay.rt_blocks), dim3(256), 0, s, b->d_indptr, b->d_indices, b->d_indptr_t, (int64_t)b->rows, b->d_norm, b->d_feat_row, f0, ff,
                               (unsigned long long*)(scr + lay.o_part), b->d_heavy[0], b->d_heavy[1], scr + lay.o_cnt, cap, b->heavy_deg, b->d_norm_c, (int2*)lay.pairs(scr, 0),
                               (int2*)lay.pairs(scr, 1), lay.first, b->d_norm_src, fd, w...);
        };
        if (b->weighted) row_tables(k_row_tables<RowW>, RowW{b->d_ew[0]}); else row_tables(k_row_tables<>);
    }
    GM_TRY(gm_balloc(b, &b->d_crow, b->n_c, s)); GM_TRY(gm_balloc(b, &b->d_cnorm, b->n_c, s));
    hipLaunchKernelGGL(k_centre_rows, dim3((b->n_c + 255) / 256), dim3(256), 0, s, b->d_sub_off, b->d_centre, nc, b->n_c, b->d_indptr, b->d_norm, b->d_crow, b->d_cnorm, scr + lay.o_cdeg, b->d_norm_c, scr + lay.o_centre, (int4*)b->d_dq_tab);
    GM_HIP(hipGetLastError());
    // ---- the one round trip
    fc.h_scr = sg.download((const int32_t*)scr, lay.ints);
    GM_REQUIRE(fc.h_scr, GM_ENOMEM, "finalize: pinned staging failed");
    tm.lap("launches");
    return GM_OK;
}
static int finalize_finish(gm_batch* b, hipStream_t s, gm_stager& sg, FinalizeCtx& fc) {      // (the stream has passed finalize_launch's downloads)
    gm_phase_timer tm("finalize-finish");
    const FinalScratch& lay = fc.lay;
    const int cap = fc.cap, first = lay.first, nc = b->centres;
    const int32_t* h_cnt = fc.h_scr + lay.o_cnt; const int32_t* h_cdeg = fc.h_scr + lay.o_cdeg; const int32_t* h_centre = fc.h_scr + lay.o_centre;
    gm_dev_free(fc.scratch, s); fc.scratch = nullptr;
    if (b->rows > 0) {
        const unsigned long long* h_counts = (const unsigned long long*)(fc.h_scr + lay.o_part);
        unsigned long long nr = 0, ne = 0, ns = 0;
        for (int k = 0; k < lay.rt_blocks; ++k) { nr += h_counts[3 * k]; ne += h_counts[3 * k + 1]; ns += h_counts[3 * k + 2]; }
        b->unfused_rows = (int64_t)nr; b->unfused_edges = (int64_t)ne; b->n_src = (int64_t)ns;
    }
    b->h_centre.assign(h_centre, h_centre + b->n_c);
    b->sched_win = gm_agg_window(b->rows, b->edges);
    std::vector<int32_t> heavy_h[2], tab_h[2];               // per orientation: sorted hub rows and their part table (for the list schedules below)
    std::vector<int32_t>&heavy0 = heavy_h[0], &tab0 = tab_h[0];
    for (int o = 0; o < 2; ++o) {
        b->n_heavy[o] = std::min(h_cnt[o], cap);
        if (b->n_heavy[o] > 0) {         // deterministic order (atomic append order is not)
            const size_t nh = b->n_heavy[o];
            std::vector<int32_t> h(nh), hd(nh);
            if ((int)nh <= first) { const int32_t* pr = lay.pairs(fc.h_scr, o); for (size_t k = 0; k < nh; ++k) { h[k] = pr[2 * k]; hd[k] = pr[2 * k + 1]; } }
            else {                       // more hub rows than the first fetch carried: one more round trip for this orientation
                const int32_t* a = sg.download(b->d_heavy[o], nh); const int32_t* d = sg.download(b->d_heavy[o] + cap, nh);
                GM_REQUIRE(a && d, GM_ENOMEM, "finalize: pinned staging failed");
                GM_HIP(hipStreamSynchronize(s));
                std::copy(a, a + nh, h.begin()); std::copy(d, d + nh, hd.begin());
            }
            sort_rows_with_degrees(h, hd, b->rows);
            if (nh > 1) GM_TRY(sg.upload(b->d_heavy[o], h));
            tm.lap("hub-sort");
            gm_agg_sched sc;
            GM_TRY(gm_agg_schedule(b, b->rows, b->sched_win, h.data(), hd.data(), b->n_heavy[o], &sc, s, &sg));
            tm.lap("schedule");
            heavy_h[o] = h; tab_h[o] = sc.tab;
            {   // stream tables: at first use (gm_agg_stream_args), from these host copies
                gm_batch::stream_pending& sp = b->spend[o];
                sp.pending = true; sp.has_tab = sc.d_hub != nullptr; sp.n_parts = sc.d_hub ? sc.parts : (int)nh;
                sp.hubs = h; sp.deg = hd; if (sp.has_tab) sp.tab = sc.tab;
            }
            b->d_sched[o] = sc.d_sched; b->sched_len[o] = sc.len; b->d_hub[o] = sc.d_hub; b->d_hub_scratch[o] = sc.d_hub_scratch; b->hub_part[o] = sc.hub_part; b->hub_words[o] = sc.hub_words; b->hub_parts[o] = sc.parts;
        } else b->spend[o].pending = true;                       // (no hub rows)
    }
    // ---- the window rows of the fused passes' partial aggregate launch as a compact ascending list + its block schedule (no host wait: the
    // list's length follows from counts the round trip above already brought: rows with more than GM_FUSE_MAXDEG in-edges minus the hub rows)
    // (the one compaction: rows of orientation indptr with lo <= degree <= hi and, with flag, its sign bit clear -> list[0 .. cap), ascending; total: see k_mid_scan)
    auto compact = [&](const int32_t* indptr, const float* flag, int lo, int hi, int32_t* list, int64_t n_cap, int32_t* total) {
        const int nb = (int)((b->rows + MID_BLOCK - 1) / MID_BLOCK);
        int32_t* d_bcnt = nullptr;
        GM_TRY(gm_alloc(&d_bcnt, (size_t)nb, s));
        hipLaunchKernelGGL(k_mid_count, dim3(nb), dim3(MID_BLOCK), 0, s, indptr, flag, (int64_t)b->rows, lo, hi, d_bcnt);
        hipLaunchKernelGGL(k_mid_scan, dim3(1), dim3(1024), 0, s, d_bcnt, nb, total, (int)n_cap);
        hipLaunchKernelGGL(k_mid_scatter, dim3(nb), dim3(MID_BLOCK), 0, s, indptr, flag, (int64_t)b->rows, lo, hi, d_bcnt, list, (int)n_cap);
        GM_HIP(hipGetLastError());
        gm_dev_free(d_bcnt, s);
        return (int)GM_OK;
    };
    // window size over a list of n rows: enough waves to fill the chip, at least two rows per wave (two rows in flight per lane group)
    auto list_window = [](int64_t n) { int win = 64; while (win > 2 && n / win < 16384) win >>= 1; return gm_knob().agg_mid_win > 0 ? gm_knob().agg_mid_win : win; };
    // hub parts of orientation o ride in a list's launch: placed after the list block nearest to the hub row's position (row id scaled to the list's n rows)
    auto list_schedule = [&](int o, int64_t n, int win, int32_t** d_sched, int32_t* len, const uint8_t* keep = nullptr) {
        std::vector<int32_t> pos(heavy_h[o].size());
        for (size_t k = 0; k < pos.size(); ++k) pos[k] = (int32_t)std::min<int64_t>(std::max<int64_t>(n, 1) - 1, (int64_t)heavy_h[o][k] * n / b->rows);
        return gm_agg_schedule_flat(b, n, win, pos.data(), (int)pos.size(), tab_h[o], d_sched, len, s, &sg, keep);
    };
    if (b->d_fuse2 && gm_knob().agg_mid_list) {
        const int64_t n_mid = b->unfused_rows - (int64_t)b->n_heavy[0];
        if (n_mid > 0 && n_mid < b->rows && h_cnt[0] <= cap) {
            GM_TRY(gm_balloc(b, &b->d_mid, (size_t)n_mid, s));
            GM_TRY(compact(b->d_indptr, nullptr, GM_FUSE_MAXDEG + 1, b->heavy_deg, b->d_mid, n_mid, nullptr));
            b->n_mid = (int32_t)n_mid;
            b->mid_win = list_window(n_mid);
            if (b->n_heavy[0] > 0 && b->d_sched[0]) GM_TRY(list_schedule(0, n_mid, b->mid_win, &b->d_sched_mid, &b->sched_len_mid));
        }
    }
    tm.lap("mid-list");
    // ---- compact lists for the row-sparse backward: centre rows and the in-edges of centres
    std::vector<int32_t> eoff(b->n_c + 1, 0);
    for (int k = 0; k < b->n_c; ++k) eoff[k + 1] = eoff[k] + h_cdeg[k];
    b->n_e1 = eoff[b->n_c];
    int32_t* d_eoff = nullptr;
    GM_TRY(gm_alloc(&d_eoff, eoff.size(), s));
    GM_TRY(sg.upload(d_eoff, eoff));
    GM_TRY(gm_balloc(b, &b->d_e1_row, b->n_e1, s)); GM_TRY(gm_balloc(b, &b->d_e1_par, b->n_e1, s)); GM_TRY(gm_balloc(b, &b->d_e1_norm, b->n_e1, s));
    if (b->weighted) GM_TRY(gm_balloc(b, &b->d_e1_coef, b->n_e1, s));
    auto centre_edges = [&](auto kern, auto... w) {
        hipLaunchKernelGGL(kern, dim3(b->n_c), dim3(64), 0, s, b->d_crow, d_eoff, b->n_c, b->d_indptr, b->d_indices, b->d_norm, b->d_e1_row, b->d_e1_par, b->d_e1_norm, w...);
    };
    if (b->weighted) centre_edges(k_centre_edges<CentreW>, CentreW{b->d_ew[0], b->d_e1_coef}); else centre_edges(k_centre_edges<>);
    GM_HIP(hipGetLastError());
    if (b->rows > 0 && b->d_norm_c) {
        GM_TRY(gm_balloc(b, &b->d_ect, (size_t)b->edges, s)); GM_TRY(gm_balloc(b, &b->d_norm_e1, (size_t)b->rows, s)); GM_TRY(gm_balloc(b, &b->d_n_e1_rows, 1, s));
        hipLaunchKernelGGL(k_e1_tables, dim3(grid_for(std::max<int64_t>(b->edges, b->rows), 4096)), dim3(256), 0, s, b->d_indices_t, (int64_t)b->edges, b->d_norm, b->d_norm_c, (int64_t)b->rows, b->d_ect, b->d_norm_e1, b->d_n_e1_rows);
        if (b->n_e1 > 0) hipLaunchKernelGGL(k_e1_rows, dim3((b->n_e1 + 255) / 256), dim3(256), 0, s, b->d_e1_row, b->n_e1, b->d_norm_e1, b->d_n_e1_rows);
        GM_HIP(hipGetLastError());
        if (b->d_fuse2 && b->d_fuse2_feat) {      // GM_DEAD_ROWS=3: the forward-only passes' source tables and keep flags over the same two row sets
            int4 *tc = nullptr, *te = nullptr, *tf = nullptr;
            GM_TRY(gm_balloc(b, &tc, (size_t)b->rows, s)); GM_TRY(gm_balloc(b, &te, (size_t)b->rows, s)); GM_TRY(gm_balloc(b, &tf, (size_t)b->rows, s));
            GM_TRY(gm_balloc(b, &b->d_obs[0], (size_t)b->rows, s)); GM_TRY(gm_balloc(b, &b->d_obs[1], (size_t)b->rows, s));
            hipLaunchKernelGGL(k_fwd_tables, dim3(grid_for(b->rows, 4096)), dim3(256), 0, s, (const int4*)b->d_fuse2, (const int4*)b->d_fuse2_feat, b->d_norm_c, b->d_norm_e1, (int64_t)b->rows,
                               tc, te, tf, b->d_obs[0], b->d_obs[1]);
            GM_HIP(hipGetLastError());
            b->d_fwd_tab[0] = tc; b->d_fwd_tab[1] = te; b->d_fwd_tab_feat = tf;
        }
        if (b->d_tiles && b->n_tiles > 0) {      // GM_DEAD_TILES: which GEMM row tiles hold a row of either set
            GM_TRY(gm_balloc(b, &b->d_tile_live[0], (size_t)b->n_tiles, s)); GM_TRY(gm_balloc(b, &b->d_tile_live[1], (size_t)b->n_tiles, s));
            hipLaunchKernelGGL(k_tile_live, dim3(b->n_tiles), dim3(GM_GEMM_BM), 0, s, b->d_tiles, b->n_tiles, b->d_norm_c, b->d_norm_e1, b->d_tile_live[0], b->d_tile_live[1]);
            GM_HIP(hipGetLastError());
        }
        // ---- the observable rows of the restricted aggregate launches as compact lists (gm_batch::obs), each with its window and, where its orientation has hub rows,
        // its block schedule.  No host wait: [0] follows from the centres' rows and in-degrees the round trip brought; [1] / [2] are sized by their bounds, and the
        // launches read their lengths on the device.  A list is taken where its bound is below half the rows today's launch walks (d_mid's, or every row)
        if (gm_knob().agg_mid_list && h_cnt[0] <= cap && h_cnt[1] <= cap) {
            const int64_t walked_fwd = b->d_mid ? b->n_mid : b->rows;
            // list k over orientation o, n rows (exact or bound): window, schedule, taken or not.  hub_keep: the orientation's hub rows that can have work in the launch,
            // where the host knows them (list 0: the hub rows that are centres) -- the others get no block; NULL: every hub row keeps its blocks, the flagged ones leave at once
            auto finish = [&](int k, int o, int64_t n, int64_t walked, const uint8_t* hub_keep) {
                gm_batch::obs_list& ol = b->obs[k];
                ol.cap = (int32_t)n; ol.win = list_window(n);
                if (2 * n > walked || (b->n_heavy[o] > 0 && !b->d_sched[o])) return (int)GM_OK;
                if (b->n_heavy[o] > 0) GM_TRY(list_schedule(o, n, ol.win, &ol.sched, &ol.sched_len, hub_keep));
                ol.take = 1;
                return (int)GM_OK;
            };
            if (b->d_obs[0]) {
                // [0]: the centre rows of GM_FUSE_MAXDEG+1 .. heavy_deg in-edges (two centres may share a row); a centre that is a hub row has its work in the hub blocks
                std::vector<int32_t> lst, hubs_c;
                for (int k = 0; k < b->n_c; ++k) {
                    const int32_t row = b->h_sub_off[k / nc] + h_centre[k];
                    if (h_cdeg[k] > b->heavy_deg) hubs_c.push_back(row); else if (h_cdeg[k] > GM_FUSE_MAXDEG) lst.push_back(row);
                }
                std::sort(lst.begin(), lst.end()); lst.erase(std::unique(lst.begin(), lst.end()), lst.end());
                std::sort(hubs_c.begin(), hubs_c.end());
                const bool hub_centre = !hubs_c.empty();
                std::vector<uint8_t> hub_keep(heavy_h[0].size());
                for (size_t k = 0; k < hub_keep.size(); ++k) hub_keep[k] = std::binary_search(hubs_c.begin(), hubs_c.end(), heavy_h[0][k]) ? 1 : 0;
                gm_batch::obs_list& ol = b->obs[0];
                ol.n = (int64_t)lst.size();
                if (lst.empty() && !hub_centre) ol.take = 2;
                else {      // (hub centres alone: an empty list whose schedule carries the hub blocks)
                    GM_TRY(gm_balloc(b, &ol.rows, lst.size(), s));
                    if (!lst.empty()) GM_TRY(sg.upload(ol.rows, lst));
                    GM_TRY(finish(0, 0, (int64_t)lst.size(), walked_fwd, hub_keep.data()));
                }
            }
            GM_TRY(gm_balloc(b, &b->obs[1].len, 2, s)); b->obs[2].len = b->obs[1].len + 1;
            GM_HIP(hipMemsetAsync(b->obs[1].len, 0, 8, s));
            if (b->d_obs[1]) {
                // [1]: at most one row per in-edge of a centre, and no more than the rows of that degree range
                const int64_t n_range = b->unfused_rows - (int64_t)b->n_heavy[0], bound = std::min<int64_t>(b->n_e1, n_range);
                if (b->n_e1 == 0 || b->unfused_rows == 0) { b->obs[1].take = 2; b->obs[1].n = 0; }
                else {      // (bound 0: hub rows alone, as above; the length word stays at its 0)
                    GM_TRY(gm_balloc(b, &b->obs[1].rows, (size_t)bound, s));
                    if (bound > 0) GM_TRY(compact(b->d_indptr, b->d_obs[1], GM_FUSE_MAXDEG + 1, b->heavy_deg, b->obs[1].rows, bound, b->obs[1].len));
                    GM_TRY(finish(1, 0, bound, walked_fwd, nullptr));
                }
            }
            {   // [2]: at most one row per in-edge of a centre, of any out-degree
                const int64_t bound = std::min<int64_t>(b->n_e1, b->rows);
                if (b->n_e1 == 0) { b->obs[2].take = 2; b->obs[2].n = 0; }
                else {
                    GM_TRY(gm_balloc(b, &b->obs[2].rows, (size_t)bound, s));
                    GM_TRY(compact(b->d_indptr_t, b->d_norm_e1, 0, INT32_MAX, b->obs[2].rows, bound, b->obs[2].len));
                    GM_TRY(finish(2, 1, bound, b->rows, nullptr));
                }
            }
        }
    }
    tm.lap("obs-lists");
    std::vector<int32_t> ccoff, ecoff, c_set_off(b->sets + 1), e_set_off(b->sets + 1);      // per set: its centres, and the in-edges of its centres
    for (int t = 0; t <= b->sets; ++t) { c_set_off[t] = b->h_set_sub_off[t] * nc; e_set_off[t] = eoff[b->h_set_sub_off[t] * nc]; }
    const std::vector<int32_t> ct = set_spans(c_set_off, GM_GEMM_BM), cc = set_spans(c_set_off, gm_wgrad_chunk_rows(c_set_off), &ccoff), ec = set_spans(e_set_off, gm_wgrad_chunk_rows(e_set_off), &ecoff);
    b->n_c_tiles = (int32_t)(ct.size() / 3); b->n_c_chunks = (int32_t)(cc.size() / 3); b->n_e1_chunks = (int32_t)(ec.size() / 3);
    GM_TRY(upload_tables(b, sg, s, {{&b->d_c_tiles, &ct}, {&b->d_c_chunks, &cc}, {&b->d_c_set_chunk_off, &ccoff}, {&b->d_e1_chunks, &ec}, {&b->d_e1_set_chunk_off, &ecoff}}));
    // ---- GM_PACK_ROWS: the centre rows and the sources of their in-edges packed per set (gm_batch::pack).  No host wait: the regions and the tile tables are sized by
    // the host's bounds -- per set its centres / the in-edges of its centres, capped by its rows -- and the launches read the tile count on the device
    if (b->rows > 0 && b->d_norm_c && b->d_norm_e1 && b->d_tiles && b->n_tiles > 0 && b->sets > 0) {
        const float* keep[2] = {b->d_norm_c, b->d_norm_e1};
        const void* src[2][2] = {{b->d_fwd_tab[0], b->d_dq_tab}, {b->d_fwd_tab[1], b->d_fwd_tab_feat}};
        for (int k = 0; k < 2; ++k) {
            gm_batch::pack_set& pk = b->pack[k];
            const std::vector<int32_t>& off = k == 0 ? c_set_off : e_set_off;
            std::vector<int32_t> base(b->sets + 1, 0);
            int32_t cap_tiles = 0;
            for (int t = 0; t < b->sets; ++t) {
                const int32_t bound = std::min<int32_t>(off[t + 1] - off[t], b->h_set_row_off[t + 1] - b->h_set_row_off[t]);
                base[t + 1] = base[t] + bound; cap_tiles += (bound + GM_GEMM_BM - 1) / GM_GEMM_BM;
            }
            int32_t* d_base = nullptr;
            GM_TRY(upload_tables(b, sg, s, {{&d_base, &base}}));
            pk.cap_rows = base[b->sets]; pk.cap_tiles = cap_tiles; pk.keep = keep[k];
            GM_TRY(gm_balloc(b, &pk.rowid, (size_t)pk.cap_rows, s)); GM_TRY(gm_balloc(b, &pk.scale, (size_t)pk.cap_rows, s));
            GM_TRY(gm_balloc(b, &pk.set_cnt, (size_t)b->sets, s)); GM_TRY(gm_balloc(b, &pk.count, 1, s));
            int32_t* tl = nullptr;
            GM_TRY(gm_balloc(b, &tl, (size_t)3 * std::max(cap_tiles, 1), s));
            for (int j = 0; j < 2; ++j) {
                pk.src_tab[j] = src[k][j];
                if (src[k][j]) { int4* d = nullptr; GM_TRY(gm_balloc(b, &d, (size_t)pk.cap_rows, s)); pk.tab[j] = d; }
            }
            hipLaunchKernelGGL(k_pack_rows, dim3(b->sets), dim3(PACK_BLOCK), 0, s, b->d_set_row_off, d_base, keep[k], (const int4*)pk.src_tab[0], (const int4*)pk.src_tab[1],
                               pk.rowid, pk.scale, (int4*)pk.tab[0], (int4*)pk.tab[1], pk.set_cnt);
            hipLaunchKernelGGL(k_pack_tiles, dim3(1), dim3(64), 0, s, pk.set_cnt, d_base, b->sets, cap_tiles, tl, pk.count);
            GM_HIP(hipGetLastError());
            pk.tiles = tl;
        }
    }
    tm.lap("pack-rows");
    gm_dev_free(d_eoff, s);
    return GM_OK;
}
// one batch, or the two of a joint build: every batch's kernels and downloads queued, ONE wait, then the host halves
static int gm_batch_finalize(gm_batch* const* bs, int n, hipStream_t s, gm_stager& sg, gm_phase_timer* tm = nullptr) {
    FinalizeCtx fc[2];
    for (int p = 0; p < n; ++p) GM_TRY(finalize_launch(bs[p], s, sg, fc[p]));
    GM_HIP(hipStreamSynchronize(s));
    if (tm) tm->lap("finalize-wait");
    for (int p = 0; p < n; ++p) GM_TRY(finalize_finish(bs[p], s, sg, fc[p]));
    return GM_OK;
}

static int batch_alloc(gm_batch* b, hipStream_t s) {
    GM_TRY(gm_balloc(b, &b->d_sub_off, b->subs + 1, s)); GM_TRY(gm_balloc(b, &b->d_set_sub_off, b->sets + 1, s));
    GM_TRY(gm_balloc(b, &b->d_set_row_off, b->sets + 1, s)); GM_TRY(gm_balloc(b, &b->d_graph, b->subs, s));
    GM_TRY(gm_balloc(b, &b->d_parent, b->rows, s)); GM_TRY(gm_balloc(b, &b->d_feat_row, b->rows, s));
    GM_TRY(gm_balloc(b, &b->d_indptr, b->rows + 1, s)); GM_TRY(gm_balloc(b, &b->d_indices, b->edges, s));
    GM_TRY(gm_balloc(b, &b->d_indptr_t, b->rows + 1, s)); GM_TRY(gm_balloc(b, &b->d_indices_t, b->edges, s));
    GM_TRY(gm_balloc(b, &b->d_centre, (size_t)b->subs * b->centres, s)); GM_TRY(gm_balloc(b, &b->d_norm, b->rows, s));
    if (b->weighted) { GM_TRY(gm_balloc(b, &b->d_ew[0], b->edges, s)); GM_TRY(gm_balloc(b, &b->d_ew[1], b->edges, s)); }
    return GM_OK;
}

static int upload_small(gm_batch* b, gm_stager& sg) {
    GM_TRY(sg.upload(b->d_sub_off, b->h_sub_off)); GM_TRY(sg.upload(b->d_set_sub_off, b->h_set_sub_off));
    GM_TRY(sg.upload(b->d_set_row_off, b->h_set_row_off)); GM_TRY(sg.upload(b->d_graph, b->h_graph));
    return GM_OK;
}
// a batch under construction: dropped with everything it holds unless the builder releases it to its caller
struct BatchDrop { void operator()(gm_batch* b) const { gm_batch_destroy(b); } };
typedef std::unique_ptr<gm_batch, BatchDrop> BatchPtr;

// One build of ONE batch (n_parts = 1) or of the two batches of a meta-batch together (n_parts = 2: seeds = [part 0 | part 1]; gm_extract_pair): the
// node-set kernel runs over all subgraphs in one launch, so does the fill kernel (k_fill serves two batches), the two finalisations queue their kernels
// back to back and share one host round trip.
struct ExPart { const int32_t* set_offsets; int32_t n_sets; int32_t n_seeds; };
// What the two extraction kernels are launched with, decided once per build.  gpath: the bitmap pair of the store's largest graph does not fit the LDS
// (beyond ~650k nodes) and lives in a per-workgroup slab of HBM.  p16: 16-bit prefix words wherever a subgraph stays below 65,536 nodes
// (GM_EXTRACT_PREF16=0: 32-bit as before).  needx: the BFS keeps its `expanded` bitmap from three hops on (reference pairs stop at two whatever h says).
struct ExPlan { bool gpath, p16, needx, sym; int Wmax; size_t Wp; int64_t cap; size_t lds_a, lds_b; };      // Wp: words of the prefix region; lds_a / lds_b: dynamic LDS of k_nodes / k_fill
static ExPlan ex_plan(const gm_store* store, int64_t cap, bool given, int link, int h) {
    ExPlan pl;
    pl.cap = cap; pl.sym = link == GM_LINK_SYMMETRIC;
    pl.Wmax = (int)((store->max_nodes + 31) >> 5);
    const size_t W = (size_t)pl.Wmax;
    pl.gpath = sizeof(uint32_t) * (2 * W + EX_BLOCK + 256 + 16) > 160 * 1024;
    pl.p16 = !pl.gpath && cap < 65536 && gm_knob().extract_pref16;
    pl.needx = !given && link != 1 && h >= 3;
    pl.Wp = pl.p16 ? (W + 1) / 2 : W;
    pl.lds_a = sizeof(uint32_t) * ((pl.gpath ? 0 : W + ((pl.p16 && !pl.needx) ? pl.Wp : W)) + EX_BLOCK + 256 + 16);
    pl.lds_b = sizeof(uint32_t) * ((pl.gpath ? 0 : W + pl.Wp) + EX_BLOCK + 16);
    return pl;
}
// The instantiations a plan takes: k_nodes in four shapes (LDS with 32-bit prefix words; LDS with 16-bit ones with / without the `expanded` bitmap; global
// bitmap), each with its symmetric-pair twin; k_fill by bitmap home and prefix width, fill_w for weighted stores (the same walk, the weights written
// beside the indices).  The LDS kernels may need more than the default dynamic LDS (gm_func_full_lds before their launch).
// Masked builds (GM_LINK_MASK_TARGET) take the same shapes with MASK set -- the same signatures, so the same three members.
struct ExKernels { decltype(&k_nodes<false>) nodes; decltype(&k_fill<false>) fill; decltype(&k_fill<false, false, false, FillW>) fill_w; };
template <bool MASK> static ExKernels ex_kernels_of(const ExPlan& pl) {
    ExKernels k = {};
    if (!pl.gpath) {
        if (pl.sym) { if (!pl.p16) k.nodes = k_nodes<false, false, true, true, MASK>; else if (pl.needx) k.nodes = k_nodes<false, true, true, true, MASK>; else k.nodes = k_nodes<false, true, false, true, MASK>; }
        else if (!pl.p16) k.nodes = k_nodes<false, false, true, false, MASK>;
        else if constexpr (MASK) k.nodes = k_nodes<false, true, false, false, true>;      // (needx without sym is node seeds, which have no target link: that shape is not instantiated)
        else if (pl.needx) k.nodes = k_nodes<false, true, true>; else k.nodes = k_nodes<false, true, false>;
        if (!pl.p16) k.fill = k_fill<false, false, MASK>; else k.fill = k_fill<false, true, MASK>;
        if (!pl.p16) k.fill_w = k_fill<false, false, MASK, FillW>; else k.fill_w = k_fill<false, true, MASK, FillW>;
    } else {
        if (pl.sym) k.nodes = k_nodes<true, false, true, true, MASK>; else k.nodes = k_nodes<true, false, true, false, MASK>;
        k.fill_w = k_fill<true, false, MASK, FillW>; k.fill = k_fill<true, false, MASK>;
    }
    return k;
}
static ExKernels ex_kernels(const ExPlan& pl, bool mask) { return mask ? ex_kernels_of<true>(pl) : ex_kernels_of<false>(pl); }
// One build: arguments, what the phases hand on, what it owns.  Leaving the scope frees the device scratch on the build's stream (behind every kernel that reads it), then drops the batches not released to the caller
struct ExBuild {
    const gm_store* store; const gm_seed_t* seeds; int n_parts; const ExPart* parts; int32_t n_seeds, split;      // seeds [0, split): part 0
    int32_t h, sample_nodes, link; uint64_t rng_seed;            // link: 0 node seeds, 1 reference pairs (h ignored), GM_LINK_SYMMETRIC: h hops around both endpoints; past the plan everything asks "two centres?" (link != 0)
    bool mask = false;                                           // GM_LINK_MASK_TARGET: ex_validate takes the bit off `link`, which is the pair mode from there on
    const int32_t* nodes_flat; const int64_t* nodes_off;         // given node lists (gm_batch_from_nodes), else NULL
    hipStream_t st; ExPlan pl; ExKernels kern; ExStore S;
    gm_stager sg;                                                // pinned staging: the build makes TWO host round trips (subgraph sizes, finalisation)
    BatchPtr bs[2];
    gm_seed_t* d_seeds = nullptr; int32_t *d_nodes = nullptr, *d_degi = nullptr, *d_dego = nullptr, *d_nsub = nullptr, *d_esub = nullptr;
    int32_t* d_given = nullptr; int64_t* d_given_off = nullptr; uint32_t* d_gbits = nullptr;      // device copy of the given node lists; bitmap slabs of the global path
    int32_t* d_eoff = nullptr; const int32_t* d_order = nullptr;                                  // the subgraphs' edge offsets per batch, and behind them k_fill's workgroup order (NULL: as seeded)
    const int32_t* nsub = nullptr; const int32_t* esub = nullptr; FillOut fo[2] = {};             // nodes / edges of every subgraph, on the host after phase A; k_fill's outputs per batch
    explicit ExBuild(hipStream_t s) : st(s), sg(s) {}
    ~ExBuild() { for (void* p : {(void*)d_gbits, (void*)d_seeds, (void*)d_nodes, (void*)d_degi, (void*)d_dego, (void*)d_nsub, (void*)d_esub, (void*)d_given, (void*)d_given_off, (void*)d_eoff}) gm_dev_free(p, st); }
};

// Arguments and seeds; *cap_out: the rows a subgraph can have (the stride of the per-subgraph scratch)
static int ex_validate(ExBuild& x, int64_t* cap_out) {
    const gm_store* store = x.store; const gm_seed_t* seeds = x.seeds; const int32_t* nodes_flat = x.nodes_flat; const int64_t* nodes_off = x.nodes_off;
    GM_REQUIRE(store && seeds, GM_EINVAL, "extract: bad arguments");
    x.n_seeds = 0;
    for (int p = 0; p < x.n_parts; ++p) {
        const ExPart& q = x.parts[p];
        GM_REQUIRE(q.set_offsets && q.n_seeds >= 1 && q.n_sets >= 1, GM_EINVAL, "extract: bad arguments");
        GM_REQUIRE(q.set_offsets[0] == 0 && q.set_offsets[q.n_sets] == q.n_seeds, GM_EINVAL, "extract: set_offsets must span [0,n_seeds]");
        x.n_seeds += q.n_seeds;
    }
    x.split = x.parts[0].n_seeds;
    const bool given = nodes_flat != nullptr;
    GM_REQUIRE(!given || x.n_parts == 1, GM_EINVAL, "extract: node lists are given per batch");
    GM_REQUIRE(x.link != GM_LINK_MASK_TARGET, GM_EINVAL, "extract: link_pred=%d is GM_LINK_MASK_TARGET alone: node seeds have no target link to mask (OR the flag onto a pair mode: 1|%d or %d|%d)",
               x.link, GM_LINK_MASK_TARGET, GM_LINK_SYMMETRIC, GM_LINK_MASK_TARGET);
    x.mask = x.link > 0 && (x.link & GM_LINK_MASK_TARGET) != 0;
    if (given) x.link = (x.link & ~GM_LINK_MASK_TARGET) ? 1 : 0;      // given node lists only need to know that there are two centres (and whether to mask)
    else if (x.link >= 0 && x.link < 2 * GM_LINK_MASK_TARGET) x.link &= ~GM_LINK_MASK_TARGET;      // the pair mode (anything else fails below as it is)
    const int32_t link = x.link, h = x.h;
    if (!given) {
        const bool sym = link == GM_LINK_SYMMETRIC;
        GM_REQUIRE(link == 0 || link == 1 || sym, GM_EINVAL, "extract: link_pred=%d is not a mode (0 node seeds, 1 reference pairs, %d symmetric pairs; |%d on a pair mode masks the target link)", link | (x.mask ? GM_LINK_MASK_TARGET : 0), GM_LINK_SYMMETRIC, GM_LINK_MASK_TARGET);
        GM_REQUIRE(!sym || (h >= 1 && h <= 3), GM_EINVAL, "extract: h=%d unsupported for symmetric pairs (h in {1,2,3} around both endpoints)", h);
        GM_REQUIRE(link || (h >= 1 && h <= 3), GM_EINVAL, "extract: h=%d unsupported (the reference defines h in {1,2,3}, sdp.py:300-311)", h);
        GM_REQUIRE(x.sample_nodes >= 1, GM_EINVAL, "extract: sample_nodes must be >= 1");
    }
    int64_t cap = 1;
    for (int k = 0; k < x.n_seeds; ++k) {
        const gm_seed_t& sd = seeds[k];
        GM_REQUIRE(sd.graph >= 0 && sd.graph < store->n_graphs, GM_EINVAL, "extract: seed %d: graph %d out of range", k, sd.graph);
        const int64_t n = store->node_off[sd.graph + 1] - store->node_off[sd.graph];
        GM_REQUIRE(sd.i >= 0 && sd.i < n, GM_EINVAL, "extract: seed %d: node %d out of range", k, sd.i);
        GM_REQUIRE(!link || (sd.j >= 0 && sd.j < n), GM_EINVAL, "extract: seed %d: second node %d out of range", k, sd.j);
        if (given) {
            const int64_t a = nodes_off[k], b = nodes_off[k + 1];
            GM_REQUIRE(b > a, GM_EINVAL, "from_nodes: subgraph %d is empty", k);
            bool has_i = false, has_j = !link;
            for (int64_t q = a; q < b; ++q) {
                GM_REQUIRE(nodes_flat[q] >= 0 && nodes_flat[q] < n, GM_EINVAL, "from_nodes: node id out of range in subgraph %d", k);
                GM_REQUIRE(q == a || nodes_flat[q] > nodes_flat[q - 1], GM_EINVAL, "from_nodes: subgraph %d not strictly ascending", k);
                has_i |= nodes_flat[q] == sd.i; has_j |= nodes_flat[q] == sd.j;
            }
            GM_REQUIRE(has_i && has_j, GM_EINVAL, "from_nodes: subgraph %d does not contain its centre(s)", k);
            cap = std::max<int64_t>(cap, b - a);
        }
    }
    *cap_out = given ? cap : std::min<int64_t>(store->max_nodes, (int64_t)x.sample_nodes + 2);
    return GM_OK;
}
// Phase A over all subgraphs, and the first round trip: the subgraphs' node and edge counts
static int ex_nodes(ExBuild& x) {
    const ExPlan& pl = x.pl; hipStream_t st = x.st; const int32_t n = x.n_seeds;
    GM_TRY(gm_alloc(&x.d_seeds, n, st));
    GM_TRY(gm_alloc(&x.d_nodes, (size_t)n * pl.cap, st)); GM_TRY(gm_alloc(&x.d_degi, (size_t)n * pl.cap, st)); GM_TRY(gm_alloc(&x.d_dego, (size_t)n * pl.cap, st));
    GM_TRY(gm_alloc(&x.d_nsub, n, st)); GM_TRY(gm_alloc(&x.d_esub, n, st));
    GM_TRY(x.sg.upload(x.d_seeds, x.seeds, sizeof(gm_seed_t) * n));
    if (x.nodes_flat) {
        const int64_t tot = x.nodes_off[n];
        GM_TRY(gm_alloc(&x.d_given, tot, st)); GM_TRY(gm_alloc(&x.d_given_off, n + 1, st));
        GM_TRY(x.sg.upload(x.d_given, x.nodes_flat, sizeof(int32_t) * tot));
        GM_TRY(x.sg.upload(x.d_given_off, x.nodes_off, sizeof(int64_t) * (n + 1)));
    }
    if (!pl.gpath) GM_TRY(gm_func_full_lds((const void*)x.kern.nodes));
    gm_prof_begin(GM_PROF_EX_NODES, st, n);
    if (pl.gpath) GM_TRY(gm_alloc(&x.d_gbits, (size_t)n * 2 * pl.Wmax, st));
    hipLaunchKernelGGL(x.kern.nodes, dim3(n), dim3(EX_BLOCK), pl.lds_a, st, x.S, x.d_seeds, n, x.h, x.sample_nodes, x.rng_seed, x.link ? 1 : 0,
                       x.d_given, x.d_given_off, (int)pl.cap, x.d_nodes, x.d_degi, x.d_dego, x.d_nsub, x.d_esub, pl.Wmax, x.d_gbits);
    gm_prof_end(GM_PROF_EX_NODES, st);
    GM_HIP(hipGetLastError());
    x.nsub = x.sg.download(x.d_nsub, (size_t)n); x.esub = x.sg.download(x.d_esub, (size_t)n);
    GM_REQUIRE(x.nsub && x.esub, GM_ENOMEM, "extract: pinned staging failed");
    GM_HIP(hipStreamSynchronize(st));
    return GM_OK;
}
// Per batch: host prefix sums, device arrays, k_fill's outputs; the edge offsets of both batches share one upload ([part 0: n0 + 1 | part 1: n1 + 1])
static int ex_size_parts(ExBuild& x) {
    const int32_t n_seeds = x.n_seeds; const int32_t* nsub = x.nsub; const int32_t* esub = x.esub;
    std::vector<int32_t> eoff;
    eoff.reserve(2 * (size_t)n_seeds + x.n_parts);          // (+ k_fill's workgroup order below: no reallocation under eoff_p)
    eoff.assign((size_t)n_seeds + x.n_parts, 0);
    int32_t* eoff_p[2] = {eoff.data(), eoff.data() + x.split + 1};
    for (int p = 0, k0 = 0; p < x.n_parts; k0 += x.parts[p].n_seeds, ++p) {
        gm_batch* b = x.bs[p].get(); const ExPart& q = x.parts[p];
        b->store = x.store; b->subs = q.n_seeds; b->sets = q.n_sets; b->centres = x.link ? 2 : 1; b->stream = x.st; b->weighted = x.store->weighted; b->mask_target = x.mask;
        batch_features(b, gm_get_hop_labels());
        b->h_sub_off.assign(q.n_seeds + 1, 0); b->h_graph.resize(q.n_seeds);
        int64_t rows = 0, edges = 0;
        for (int k = 0; k < q.n_seeds; ++k) {
            const int gk = k0 + k;
            GM_REQUIRE(nsub[gk] > 0 && esub[gk] >= 0, GM_ERANGE, "extract: subgraph %d failed on device (nodes=%d, edges=%d, cap=%lld)", gk, nsub[gk], esub[gk], (long long)x.pl.cap);
            rows += nsub[gk]; edges += esub[gk];
            GM_REQUIRE(rows <= INT32_MAX - 2 && edges <= INT32_MAX - 2, GM_ERANGE, "extract: batch exceeds 2^31 rows/edges; split the meta-batch");
            b->h_sub_off[k + 1] = (int32_t)rows; eoff_p[p][k + 1] = (int32_t)edges; b->h_graph[k] = x.seeds[gk].graph;
        }
        b->rows = rows; b->edges = edges;
        b->h_set_sub_off.assign(q.set_offsets, q.set_offsets + q.n_sets + 1);
        b->h_set_row_off.resize(q.n_sets + 1);
        for (int s = 0; s <= q.n_sets; ++s) b->h_set_row_off[s] = b->h_sub_off[q.set_offsets[s]];
        GM_TRY(batch_alloc(b, x.st));
        GM_TRY(upload_small(b, x.sg));
    }
    // k_fill's workgroup order rides in the same upload: subgraphs by edge count, largest first (64 linear buckets: coarse is enough, and O(n))
    const size_t o_order = eoff.size();
    const bool lpt = n_seeds >= 512;                      // (more subgraphs than workgroup slots in half a round: 0.156 -> 0.145 ms at the arxiv shape, profiles/r06_experiments_not_shipped.txt H)
    if (lpt) {
        int emax = 1;
        for (int k = 0; k < n_seeds; ++k) emax = std::max(emax, esub[k]);
        int cnt[65] = {0};
        auto bucket = [&](int e) { return 63 - (int)((int64_t)e * 63 / emax); };             // 0 = largest
        for (int k = 0; k < n_seeds; ++k) ++cnt[bucket(esub[k]) + 1];
        for (int q = 0; q < 64; ++q) cnt[q + 1] += cnt[q];
        eoff.resize(o_order + n_seeds);
        for (int k = 0; k < n_seeds; ++k) eoff[o_order + cnt[bucket(esub[k])]++] = k;
    }
    GM_TRY(gm_alloc(&x.d_eoff, eoff.size(), x.st));
    GM_TRY(x.sg.upload(x.d_eoff, eoff));
    x.d_order = lpt ? x.d_eoff + o_order : nullptr;
    for (int p = 0; p < x.n_parts; ++p) {
        gm_batch* b = x.bs[p].get();
        x.fo[p] = FillOut{b->d_sub_off, x.d_eoff + (p ? x.split + 1 : 0), b->d_parent, b->d_feat_row, b->d_norm, b->d_indptr, b->d_indices, b->d_indptr_t, b->d_indices_t, b->d_centre};
    }
    if (x.n_parts == 1) x.fo[1] = x.fo[0];
    return GM_OK;
}
// Phase B over all subgraphs; weighted stores: the weights ride in k_fill's last argument, and the weighted in-degree's norm of every batch follows
static int ex_fill(ExBuild& x) {
    const ExPlan& pl = x.pl; hipStream_t st = x.st; const int32_t n = x.n_seeds;
    const bool weighted = x.store->weighted;
    if (!pl.gpath) GM_TRY(gm_func_full_lds(weighted ? (const void*)x.kern.fill_w : (const void*)x.kern.fill));
    auto launch = [&](auto kern, auto... w) {
        hipLaunchKernelGGL(kern, dim3(n), dim3(EX_BLOCK), pl.lds_b, st, x.S, x.d_seeds, n, x.link ? 1 : 0, (int)pl.cap, x.d_nodes, x.d_degi, x.d_dego, x.fo[0], x.fo[1], (int)x.split,
                           pl.Wmax, x.d_gbits, x.d_order, w...);
    };
    gm_prof_begin(GM_PROF_EX_FILL, st, n);
    if (weighted) {
        gm_batch* b0 = x.bs[0].get(); gm_batch* b1 = x.bs[x.n_parts - 1].get();
        const FillW fw{x.store->d_in_w, x.store->d_out_w, {b0->d_ew[0], b0->d_ew[1]}, {b1->d_ew[0], b1->d_ew[1]}};
        launch(x.kern.fill_w, fw);
        for (int p = 0; p < x.n_parts; ++p)
            if (gm_batch* b = x.bs[p].get(); b->rows > 0) hipLaunchKernelGGL(k_weighted_norm, dim3(grid_for(b->rows, 2048)), dim3(256), 0, st, b->d_indptr, b->d_ew[0], (int64_t)b->rows, b->d_norm);
    } else launch(x.kern.fill);
    gm_prof_end(GM_PROF_EX_FILL, st);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
static int extract_impl(const gm_store_t* store, const gm_seed_t* seeds, int n_parts, const ExPart* parts, int32_t h, int32_t sample_nodes, uint64_t rng_seed,
                        int32_t link, const int32_t* nodes_flat, const int64_t* nodes_off, void* stream, gm_batch_t** outs) {
    GM_REQUIRE(outs && (n_parts == 1 || n_parts == 2), GM_EINVAL, "extract: out is NULL");
    for (int p = 0; p < n_parts; ++p) outs[p] = nullptr;
    gm_phase_timer tm("extract");
    ExBuild x((hipStream_t)stream);
    x.store = store; x.seeds = seeds; x.n_parts = n_parts; x.parts = parts; x.h = h; x.sample_nodes = sample_nodes; x.link = link; x.rng_seed = rng_seed;
    x.nodes_flat = nodes_flat; x.nodes_off = nodes_off;
    int64_t cap = 1;
    GM_TRY(ex_validate(x, &cap));
    x.pl = ex_plan(store, cap, nodes_flat != nullptr, x.link, h); x.kern = ex_kernels(x.pl, x.mask);
    x.S = ExStore{store->d_node_off, store->d_in_ptr, store->d_in_idx, store->d_out_ptr, store->d_out_idx, store->symmetric ? 1 : 0};
    for (int p = 0; p < n_parts; ++p) x.bs[p].reset(new gm_batch());
    tm.lap("validate");
    GM_TRY(ex_nodes(x));
    tm.lap("k_nodes+sizes");
    GM_TRY(ex_size_parts(x));
    GM_TRY(ex_fill(x));
    tm.lap("alloc+k_fill");
    gm_batch* const bs[2] = {x.bs[0].get(), x.bs[1].get()};
    gm_prof_begin(GM_PROF_EX_FINAL, x.st, 1);
    GM_TRY(gm_batch_finalize(bs, n_parts, x.st, x.sg, &tm));
    gm_prof_end(GM_PROF_EX_FINAL, x.st);
    tm.lap("finalize");
    for (int p = 0; p < n_parts; ++p) outs[p] = x.bs[p].release();
    return GM_OK;
}

extern "C" int gm_extract(const gm_store_t* store, const gm_seed_t* seeds, int32_t n_seeds, const int32_t* set_offsets, int32_t n_sets,
                          int32_t h, int32_t sample_nodes, uint64_t rng_seed, int32_t link_pred, void* stream, gm_batch_t** out) {
    GM_REQUIRE(out, GM_EINVAL, "extract: out is NULL");
    const ExPart part{set_offsets, n_sets, n_seeds};
    return extract_impl(store, seeds, 1, &part, h, sample_nodes, rng_seed, link_pred, nullptr, nullptr, stream, out);
}

extern "C" int gm_extract_pair(const gm_store_t* store, const gm_seed_t* seeds_a, int32_t n_seeds_a, const int32_t* set_offsets_a, int32_t n_sets_a,
                               const gm_seed_t* seeds_b, int32_t n_seeds_b, const int32_t* set_offsets_b, int32_t n_sets_b,
                               int32_t h, int32_t sample_nodes, uint64_t rng_seed, int32_t link_pred, void* stream, gm_batch_t** out_a, gm_batch_t** out_b) {
    GM_REQUIRE(out_a && out_b && seeds_a && seeds_b && n_seeds_a >= 1 && n_seeds_b >= 1, GM_EINVAL, "extract_pair: bad arguments");
    *out_a = nullptr; *out_b = nullptr;
    std::vector<gm_seed_t> all((size_t)n_seeds_a + n_seeds_b);
    std::copy(seeds_a, seeds_a + n_seeds_a, all.begin()); std::copy(seeds_b, seeds_b + n_seeds_b, all.begin() + n_seeds_a);
    const ExPart parts[2] = {{set_offsets_a, n_sets_a, n_seeds_a}, {set_offsets_b, n_sets_b, n_seeds_b}};
    gm_batch_t* outs[2] = {nullptr, nullptr};
    const int rc = extract_impl(store, all.data(), 2, parts, h, sample_nodes, rng_seed, link_pred, nullptr, nullptr, stream, outs);
    *out_a = outs[0]; *out_b = outs[1];
    return rc;
}

extern "C" int gm_batch_from_nodes(const gm_store_t* store, const gm_seed_t* seeds, int32_t n_seeds, const int32_t* set_offsets,
                                   int32_t n_sets, const int32_t* nodes_flat, const int64_t* nodes_off, int32_t link_pred, void* stream,
                                   gm_batch_t** out) {
    GM_REQUIRE(out && nodes_flat && nodes_off, GM_EINVAL, "from_nodes: node lists are NULL");
    const ExPart part{set_offsets, n_sets, n_seeds};
    return extract_impl(store, seeds, 1, &part, 1, 1, 0, link_pred, nodes_flat, nodes_off, stream, out);
}

extern "C" int gm_batch_concat(const gm_batch_t* const* parts, int32_t n_parts, void* stream, gm_batch_t** out) {
    GM_REQUIRE(out, GM_EINVAL, "concat: out is NULL");
    *out = nullptr;
    GM_REQUIRE(parts && n_parts >= 1, GM_EINVAL, "concat: no parts");
    hipStream_t st = (hipStream_t)stream;
    const gm_batch* p0 = parts[0];
    int64_t rows = 0, edges = 0, subs = 0, sets = 0;
    for (int p = 0; p < n_parts; ++p) {
        const gm_batch* q = parts[p];
        GM_REQUIRE(!(q && p0) || q->weighted == p0->weighted, GM_EINVAL, "concat: part %d is %s but part 0 is %s: weighted and unweighted batches cannot be concatenated", p,
                   q->weighted ? "weighted" : "unweighted", p0->weighted ? "weighted" : "unweighted");
        GM_REQUIRE(!(q && p0) || q->hop_D == p0->hop_D, GM_EINVAL, "concat: part %d has hop labels D=%d but part 0 has D=%d: parts must all be labelled with the same D, or all unlabelled", p,
                   q->hop_D, p0->hop_D);
        GM_REQUIRE(!(q && p0) || q->mask_target == p0->mask_target, GM_EINVAL, "concat: part %d is %s but part 0 is %s: parts must all be built with GM_LINK_MASK_TARGET, or all without", p,
                   q->mask_target ? "target-masked" : "unmasked", p0->mask_target ? "target-masked" : "unmasked");
        GM_REQUIRE(q && p0 && q->store == p0->store && q->centres == p0->centres, GM_EINVAL, "concat: part %d has a different store or centre count", p);
        rows += q->rows; edges += q->edges; subs += q->subs; sets += q->sets;
    }
    GM_REQUIRE(rows <= INT32_MAX - 2 && edges <= INT32_MAX - 2, GM_ERANGE, "concat: batch exceeds 2^31 rows/edges");
    BatchPtr held(new gm_batch());
    gm_batch* b = held.get();
    b->store = p0->store; b->centres = p0->centres; b->stream = st;
    b->rows = rows; b->edges = edges; b->subs = (int32_t)subs; b->sets = (int32_t)sets;
    b->h_sub_off.assign(1, 0); b->h_set_sub_off.assign(1, 0); b->h_set_row_off.assign(1, 0);
    b->weighted = p0->weighted; b->mask_target = p0->mask_target;
    batch_features(b, p0->hop_D);      // (labelled parts: the finalisation labels the concatenated subgraphs again -- the same labels, the concatenated table)
    GM_TRY(batch_alloc(b, st));
    int64_t r0 = 0, e0 = 0; int32_t s0 = 0;
    auto cpy = [&](int32_t* dst, const int32_t* src, int64_t n, int32_t add) {
        if (n > 0) hipLaunchKernelGGL(k_copy_add, dim3(grid_for(n, 1024)), dim3(256), 0, st, dst, src, n, add);
    };
    for (int p = 0; p < n_parts; ++p) {
        const gm_batch* q = parts[p];
        cpy(b->d_parent + r0, q->d_parent, q->rows, 0); cpy(b->d_feat_row + r0, q->d_store_row, q->rows, 0);
        cpy((int32_t*)b->d_norm + r0, (const int32_t*)q->d_norm, q->rows, 0);
        cpy(b->d_indptr + r0, q->d_indptr, q->rows + (p == n_parts - 1 ? 1 : 0), (int32_t)e0);
        cpy(b->d_indptr_t + r0, q->d_indptr_t, q->rows + (p == n_parts - 1 ? 1 : 0), (int32_t)e0);
        cpy(b->d_indices + e0, q->d_indices, q->edges, (int32_t)r0); cpy(b->d_indices_t + e0, q->d_indices_t, q->edges, (int32_t)r0);
        if (b->weighted) { cpy((int32_t*)b->d_ew[0] + e0, (const int32_t*)q->d_ew[0], q->edges, 0); cpy((int32_t*)b->d_ew[1] + e0, (const int32_t*)q->d_ew[1], q->edges, 0); }
        cpy(b->d_centre + (int64_t)s0 * b->centres, q->d_centre, (int64_t)q->subs * b->centres, 0);
        for (int k = 1; k <= q->subs; ++k) b->h_sub_off.push_back((int32_t)(r0 + q->h_sub_off[k]));
        for (int k = 1; k <= q->sets; ++k) { b->h_set_sub_off.push_back(s0 + q->h_set_sub_off[k]); b->h_set_row_off.push_back((int32_t)(r0 + q->h_set_row_off[k])); }
        b->h_graph.insert(b->h_graph.end(), q->h_graph.begin(), q->h_graph.end());
        r0 += q->rows; e0 += q->edges; s0 += q->subs;
    }
    GM_REQUIRE(hipGetLastError() == hipSuccess, GM_EHIP, "concat: copy kernel launch failed");
    gm_stager sg(st);
    GM_TRY(upload_small(b, sg));
    GM_TRY(gm_batch_finalize(&b, 1, st, sg));
    *out = held.release();
    return GM_OK;
}

int gm_gather_rows(const gm_batch* b, const int32_t* feat_row, int64_t n, int F, float* out, hipStream_t st) {
    if (n <= 0) return GM_OK;          // F: columns copied (feat_dim, or feat_ld for the padded internal model); feat_row: rows of the batch's feature table
    hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(n * F, 256 * 8)), dim3(256), 0, st, b->feat, (int64_t)b->feat_ld, feat_row, out, n, F);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

extern "C" int gm_gather_features(const gm_batch_t* b, float* x_out, void* stream) {
    GM_REQUIRE(b && x_out, GM_EINVAL, "gather_features: NULL argument");
    return gm_gather_rows(b, b->d_feat_row, b->rows, b->feat_dim, x_out, (hipStream_t)stream);
}
