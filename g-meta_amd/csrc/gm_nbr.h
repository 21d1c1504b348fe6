// The neighbour index (nbr_index.hip; gm_store in gm_internal.h) as the kernels see it: one graph's view, the search of a row, the adjacency test, the
// canonical form of a pair and the intersection of two rows.  Included by the translation units that read the index (pair_scores.hip, candidates.hip,
// pair_walks.hip, pair_pagerank.hip, pair_distance.hip).  Every meaning bits depend on -- the tie rule, the symmetric rows -- is stated here once.
#pragma once
#include "gm_internal.h"

// one parent graph of a store inside the neighbour index: rows by LOCAL node id, offsets global (into idx), neighbours local
struct gm_nbr_graph {
    const int64_t* ptr;          // gm_store::d_nbr_ptr + node_off[g]   [N + 1]
    const int32_t* idx;          // gm_store::d_nbr_idx
    int64_t N;
};
gm_nbr_graph gm_nbr_graph_of(const gm_store* s, int32_t g);      // (host; g in range, the index built: gm_nbr_index)

// v in the ascending row[0 .. len)
__device__ __forceinline__ bool gm_nbr_has(const int32_t* __restrict__ row, int32_t len, int32_t v) {
    int32_t lo = 0, hi = len;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t x = row[mid];
        if (x == v) return true;
        if (x < v) lo = mid + 1; else hi = mid;
    }
    return false;
}

// a pair as the kernels see it: canonical (u, v), u <= v -- (a, b) and (b, a) run the same instructions on the same data --, the shorter of the two rows X
// (a tie takes the smaller id's row) and the other row T
struct gm_nbr_pair {
    const int32_t* X; const int32_t* T;
    int32_t dx, dt, u, v, du, dv;
    bool in;                      // both ids inside the graph
};
__device__ __forceinline__ gm_nbr_pair gm_nbr_pair_of(const gm_nbr_graph& G, const int32_t* __restrict__ pairs, int64_t p) {
    gm_nbr_pair w = {nullptr, nullptr, 0, 0, -1, -1, 0, 0, false};
    const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    w.in = a >= 0 && a < G.N && b >= 0 && b < G.N;
    if (!w.in) return w;
    w.u = a < b ? a : b; w.v = a < b ? b : a;
    const int64_t u0 = G.ptr[w.u], v0 = G.ptr[w.v];
    w.du = (int32_t)(G.ptr[w.u + 1] - u0); w.dv = (int32_t)(G.ptr[w.v + 1] - v0);
    const bool u_short = w.du <= w.dv;
    w.X = G.idx + (u_short ? u0 : v0); w.T = G.idx + (u_short ? v0 : u0);
    w.dx = u_short ? w.du : w.dv; w.dt = u_short ? w.dv : w.du;
    return w;
}

// a and b are distinct, inside the graph and neighbours: b in a's row  (b in a's row <=> a in b's row: the rows are symmetric, so the orientation of the
// pair and which of the two rows is searched cannot change the answer)
__device__ __forceinline__ bool gm_nbr_adjacent(const gm_nbr_graph& G, int32_t a, int32_t b) {
    if ((a == b) | (a < 0) | (a >= G.N) | (b < 0) | (b >= G.N)) return false;      // (one branch for the five tests: no memory is read)
    const int64_t a0 = G.ptr[a];
    return gm_nbr_has(G.idx + a0, (int32_t)(G.ptr[a + 1] - a0), b);
}
// the same for a loaded pair: the search runs in the shorter row, which the kernel reads anyway (by value: the kernels' instruction order is the inline test's)
__device__ __forceinline__ bool gm_nbr_adjacent(gm_nbr_pair w) { return w.u != w.v && gm_nbr_has(w.X, w.dx, w.du <= w.dv ? w.v : w.u); }

// The lane's fold over the ids common to the ascending rows A[0 .. na) and B[0 .. nb): acc = hit(acc, z) for every such z the lane meets, by a group of L
// lanes (every lane of the group calls it with the same rows; lane = its number in the group).  The group strides over A if it is not longer than B, else over
// B -- consecutive lanes read consecutive ids: one coalesced load per step -- and each lane binary-searches its id in the other row: log2(length) dependent
// loads, the upper levels shared by the whole group in L1 / L2.  A lane meets its ids in ascending order of the strided row: which row that is decides the
// order of a float sum made in `hit`.  (The running value is passed and returned, not captured by reference: a captured counter stays in memory until the
// compiler's second scalar-replacement pass, and the search loop around it came out with more branches and scalar registers.)
template <int L, class Acc, class Hit>
__device__ __forceinline__ Acc gm_nbr_common(const int32_t* A, int32_t na, const int32_t* B, int32_t nb, int lane, Acc acc, Hit hit) {
    const bool a_short = na <= nb;
    const int32_t* __restrict__ S = a_short ? A : B;
    const int32_t* __restrict__ R = a_short ? B : A;
    const int32_t ns = a_short ? na : nb, nr = a_short ? nb : na;
    for (int32_t j = lane; j < ns; j += L) {
        const int32_t z = S[j];
        if (gm_nbr_has(R, nr, z)) acc = hit(acc, z);
    }
    return acc;
}
