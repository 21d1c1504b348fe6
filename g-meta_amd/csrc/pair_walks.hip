// Walk counts of node pairs (gm_store_pair_walks: the numbers of walks of length 1, 2 and 3 between the two nodes in the distinct-neighbour graph -- what the
// local path index and the truncated Katz index are made of).  The DEFINITION is in include/gmeta_hip.h; tests/path_walk_ref.py restates it with Python sets.
// This file is how it is computed, over the neighbour index (nbr_index.hip; gm_nbr.h):
//   the work    w3(u, v) = sum over z in G(x) of |G(z) & G(t)|, x the endpoint with the shorter row (a tie: the smaller id), t the other: one row intersection
//               per OUTER entry z.  A leaf pair is a few loads, a pair of hubs tens of thousands of intersections, so the outer row is cut into WORK ITEMS of
//               at most C entries (gm_set_tuning("walk_chunk")) and no lane group walks more than C of them in a row.
//   one item    walk_item<L>: a group of L lanes.  L outer entries at a time: every lane loads one z, its row bounds and searches z in G(t) (the w2 term), then
//               the group takes the L inner rows in turn (bounds by shuffle) -- its lanes stride the SHORTER of G(z) and G(t) and binary-search the longer
//               (gm_nbr_common, as k_pair_scores does).  Lane partials meet in a butterfly over the group.
//   light pairs k_pair_walks<L>: one group per pair.  A pair whose outer row holds at most C entries is one item: the group sums it and stores the row
//               (w1, w2, w3 + mask correction) plainly.  A heavier pair gets its row SEEDED (w1, 0, mask correction: a negative start value) and its index appended
//               to the call's heavy list through a counter; a second counter adds up the items.
//   heavy pairs the host reads the two counters back (24 bytes, the one round trip of the call) and, where there are heavy pairs, launches k_walk_expand (a group
//               per heavy pair writes its (pair, chunk) items at a base taken from a third counter) and k_walk_items<L> (a group per item: the on-chip sum, then ONE
//               64-bit integer atomic add per column and item onto the seeded row).  Integer adds commute: list order, item order and arrival order cannot
//               change a bit of the result.
// No float arithmetic in this file, no LDS, no scratch memory.  Everything runs on the caller's stream; scratch comes from the stream-ordered pool.
#include "gm_nbr.h"

#define GM_WALK_THREADS 256
#define GM_WALK_COLS 3
#define GM_WALK_EXPAND_LANES 16           // lanes per heavy pair of k_walk_expand

typedef unsigned long long walk_u64;

__device__ __forceinline__ int64_t walk_items_of(int32_t dx, int32_t C) { return ((int64_t)dx + C - 1) / C; }

// The outer entries X[zb .. ze) against the row T, by one group of L lanes (every lane of the group calls it with the same arguments): the lane's share of
// sum [z in T] (*w2) and of sum |G(z) & T| (*w3).  The loops' bounds are the same in every lane of the group, so the shuffles find their source lanes active.
template <int L>
__device__ __forceinline__ void walk_item(const gm_nbr_graph& G, const int32_t* __restrict__ X, int64_t zb, int64_t ze, const int32_t* __restrict__ T, int32_t dt, int lane,
                                          int32_t* w2, int64_t* w3) {
    int32_t c2 = 0; int64_t c3 = 0;
    for (int64_t base = zb; base < ze; base += L) {
        const int64_t i = base + lane;
        int64_t z0 = 0; int32_t dz = 0;
        if (i < ze) {
            const int32_t z = X[i];
            z0 = G.ptr[z]; dz = (int32_t)(G.ptr[z + 1] - z0);
            if (gm_nbr_has(T, dt, z)) ++c2;
        }
        const int cnt = (int)(ze - base < L ? ze - base : L);
        for (int k = 0; k < cnt; ++k) {
            const int64_t s0 = __shfl(z0, k, L);
            const int32_t ds = __shfl(dz, k, L);
            const int32_t* __restrict__ Z = G.idx + s0;
            c3 += gm_nbr_common<L>(Z, ds, T, dt, lane, (int32_t)0, [](int32_t c, int32_t) { return c + 1; });
        }
    }
    *w2 = c2; *w3 = c3;
}

template <int L> __device__ __forceinline__ void walk_butterfly(int32_t& w2, int64_t& w3) {
#pragma unroll
    for (int m = L / 2; m >= 1; m >>= 1) { w2 += __shfl_xor(w2, m, L); w3 += __shfl_xor(w3, m, L); }
}

// cnt[0]: heavy pairs so far (slots of `heavy`), cnt[1]: their items.  out rows of every pair: the result (light) or the seed (heavy)
template <int L>
__global__ void __launch_bounds__(GM_WALK_THREADS) k_pair_walks(gm_nbr_graph G, const int32_t* __restrict__ pairs, int64_t n, int mask, int32_t C, int64_t* __restrict__ out,
                                                                 int32_t* __restrict__ heavy, walk_u64* cnt) {
    const int64_t p = ((int64_t)blockIdx.x * GM_WALK_THREADS + threadIdx.x) / L;      // the group's pair: a group is live or idle as a whole
    const int lane = (int)threadIdx.x & (L - 1);
    const bool live = p < n;
    int32_t w1 = 0, w2 = 0; int64_t w3 = 0, corr = 0;
    bool is_heavy = false; int64_t items = 0;
    if (live) {
        const gm_nbr_pair w = gm_nbr_pair_of(G, pairs, p);
        if (w.in) {
            const bool adj = gm_nbr_adjacent(w);
            if (adj && mask) corr = -((int64_t)w.du + w.dv - 1);                               // the walks of S^3 that use the edge {u, v}
            else w1 = adj ? 1 : 0;
            is_heavy = w.dx > C;
            if (is_heavy) items = walk_items_of(w.dx, C);
            else walk_item<L>(G, w.X, 0, w.dx, w.T, w.dt, lane, &w2, &w3);
        }
    }
    walk_butterfly<L>(w2, w3);
    if (!live) return;
    if (lane < GM_WALK_COLS) out[GM_WALK_COLS * p + lane] = lane == 0 ? (int64_t)w1 : lane == 1 ? (int64_t)w2 : w3 + corr;      // (heavy: w2 = w3 = 0, the seed)
    if (is_heavy && lane == 0) {
        heavy[atomicAdd(&cnt[0], 1ull)] = (int32_t)p;
        atomicAdd(&cnt[1], (walk_u64)items);
    }
}

// one group per heavy pair: its items (pair, chunk) at a base from cnt[2]
__global__ void __launch_bounds__(GM_WALK_THREADS) k_walk_expand(gm_nbr_graph G, const int32_t* __restrict__ pairs, int32_t C, const int32_t* __restrict__ heavy, int64_t n_heavy,
                                                                  int64_t n_items, walk_u64* cnt, int2* __restrict__ item) {
    const int64_t h = ((int64_t)blockIdx.x * GM_WALK_THREADS + threadIdx.x) / GM_WALK_EXPAND_LANES;
    const int lane = (int)threadIdx.x & (GM_WALK_EXPAND_LANES - 1);
    if (h >= n_heavy) return;
    const int32_t p = heavy[h];
    const gm_nbr_pair w = gm_nbr_pair_of(G, pairs, p);
    const int64_t items = walk_items_of(w.dx, C);
    walk_u64 base = 0;
    if (lane == 0) base = atomicAdd(&cnt[2], (walk_u64)items);
    base = __shfl(base, 0, GM_WALK_EXPAND_LANES);
    for (int64_t i = lane; i < items; i += GM_WALK_EXPAND_LANES)
        if ((int64_t)base + i < n_items) item[base + i] = make_int2(p, (int32_t)i);      // (the bound holds by construction: the two kernels count the same items)
}

// one group per item: the on-chip sum of its outer entries, then one integer atomic add per column onto the pair's seeded row
template <int L>
__global__ void __launch_bounds__(GM_WALK_THREADS) k_walk_items(gm_nbr_graph G, const int32_t* __restrict__ pairs, int32_t C, const int2* __restrict__ item, int64_t n_items,
                                                                 int64_t* out) {
    const int64_t it = ((int64_t)blockIdx.x * GM_WALK_THREADS + threadIdx.x) / L;
    const int lane = (int)threadIdx.x & (L - 1);
    const bool live = it < n_items;
    int32_t w2 = 0; int64_t w3 = 0; int64_t p = 0;
    if (live) {
        const int2 e = item[it];
        p = e.x;
        const gm_nbr_pair w = gm_nbr_pair_of(G, pairs, p);
        const int64_t zb = (int64_t)e.y * C, ze = zb + C < w.dx ? zb + C : w.dx;
        walk_item<L>(G, w.X, zb, ze, w.T, w.dt, lane, &w2, &w3);
    }
    walk_butterfly<L>(w2, w3);
    if (!live || lane != 0) return;
    atomicAdd((walk_u64*)&out[GM_WALK_COLS * p + 1], (walk_u64)(int64_t)w2);
    atomicAdd((walk_u64*)&out[GM_WALK_COLS * p + 2], (walk_u64)w3);
}

// Lanes and outer entries per work item.  Measured on preferential-attachment graphs of mean distinct degree 2 to 554, edges + as many negatives
// (profiles/pair_walks.txt).  A LONG pair list is throughput work: 32 lanes with items of 32 entries are fastest up to a mean distinct degree of 14 (a 16-lane
// group was ahead at one point of the sweep only, by 2 %, and is not built), 64 lanes with items of 64 from 32 upwards.  A SHORT list (100,000 pairs) ends on the
// items of its heaviest pairs, whatever the density: 64 lanes and items of 16 entries were fastest on every graph, by up to 2x over the long-list choice.
#define GM_WALK_SHORT_LIST (1 << 17)
static int walk_lanes_for(const gm_store* s, int32_t g, int64_t n) {
    const int64_t N = s->node_off[g + 1] - s->node_off[g], nnz = s->nbr_off[g + 1] - s->nbr_off[g];
    return n <= GM_WALK_SHORT_LIST || nnz > 24 * N ? 64 : 32;
}
static int32_t walk_chunk_for(int64_t n, int lanes) { return n <= GM_WALK_SHORT_LIST ? 16 : lanes; }

static unsigned walk_grid(int64_t groups, int lanes) { return (unsigned)((groups * lanes + GM_WALK_THREADS - 1) / GM_WALK_THREADS); }

extern "C" int32_t gm_store_pair_walks(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, int64_t* d_out, void* stream) {
    const char* what = "gm_store_pair_walks";
    GM_TRY(gm_store_call_check(what, s, g, "n", n, flags));
    const int chunk_knob = gm_knob().walk_chunk, forced = gm_knob().walk_lanes;
    GM_REQUIRE(chunk_knob >= 0, GM_EINVAL, "%s: walk_chunk = %d", what, chunk_knob);
    GM_REQUIRE(forced == 0 || forced == 32 || forced == 64, GM_EINVAL,
               "%s: walk_lanes = %d; the kernels are built for 32 and 64 lanes per work item (0: the library's choice)", what, forced);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out, GM_EINVAL, "%s: NULL argument", what);
    GM_TRY(gm_nbr_index(s));
    const int L = forced ? forced : walk_lanes_for(s, g, n);                 // (the library's choice reads the index's row lengths)
    const int32_t C = chunk_knob > 0 ? chunk_knob : walk_chunk_for(n, L);
    const int mask = flags & GM_PAIR_MASK_TARGET;
    hipStream_t st = (hipStream_t)stream;
    const gm_nbr_graph G = gm_nbr_graph_of(s, g);

    gm_scratch sc(st);
    walk_u64* cnt = nullptr; int32_t* heavy = nullptr; int2* item = nullptr;
    GM_TRY(sc.take(&cnt, 3));
    GM_TRY(sc.take(&heavy, (size_t)n));
    GM_HIP(hipMemsetAsync(cnt, 0, 3 * sizeof(walk_u64), st));
    {
        const dim3 grid(walk_grid(n, L)), block(GM_WALK_THREADS);             // n <= 2^31 - 1 pairs of at most 64 lanes: below 2^29 blocks
        if (L == 32) hipLaunchKernelGGL(k_pair_walks<32>, grid, block, 0, st, G, d_pairs, n, mask, C, d_out, heavy, cnt);
        else hipLaunchKernelGGL(k_pair_walks<64>, grid, block, 0, st, G, d_pairs, n, mask, C, d_out, heavy, cnt);
        GM_HIP(hipGetLastError());
    }
    gm_stager sg(st);
    const walk_u64* h_cnt = sg.download((const walk_u64*)cnt, 2);
    GM_REQUIRE(h_cnt, GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(st));
    const int64_t n_heavy = (int64_t)h_cnt[0], n_items = (int64_t)h_cnt[1];
    if (n_heavy == 0) return GM_OK;
    GM_REQUIRE(n_items <= (int64_t)INT32_MAX / 2, GM_ERANGE, "%s: %lld work items at walk_chunk = %d; the item launch holds 2^30 at most", what, (long long)n_items, (int)C);
    GM_TRY(sc.take(&item, (size_t)n_items));
    hipLaunchKernelGGL(k_walk_expand, dim3(walk_grid(n_heavy, GM_WALK_EXPAND_LANES)), dim3(GM_WALK_THREADS), 0, st, G, d_pairs, C, (const int32_t*)heavy, n_heavy, n_items, cnt, item);
    GM_HIP(hipGetLastError());
    {
        const dim3 grid(walk_grid(n_items, L)), block(GM_WALK_THREADS);       // at most 2^30 items of at most 64 lanes: 2^28 blocks
        if (L == 32) hipLaunchKernelGGL(k_walk_items<32>, grid, block, 0, st, G, d_pairs, C, (const int2*)item, n_items, d_out);
        else hipLaunchKernelGGL(k_walk_items<64>, grid, block, 0, st, G, d_pairs, C, (const int2*)item, n_items, d_out);
        GM_HIP(hipGetLastError());
    }
    return GM_OK;
}
