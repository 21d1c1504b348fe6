// The frame of a call that runs one column per (source, excluded node) over the neighbour index, shared by pair_pagerank.hip and pair_distance.hip.  A column
// is a pair (s, x): s the source, x = -1 or the node whose edge {s, x} the column's graph lacks.  What is here once:
//   the call    gm_col_call: stream, graph and the two knobs in force (columns per round B, entries per hub segment C); gm_col_setup checks the knobs and fills it.
//   plans       gm_col_plan_of forms the DISTINCT columns of a call's output entries and the order the entries leave in; gm_col_sources (an entry per source)
//               and gm_col_pairs (one or two entries per pair) read a call's input back, plan it and upload the plan; gm_col_span: the entries of one round.
//   groups      gm_col_pair_groups cuts a call's pairs (gm_col_pairs_read) into groups of a bounded number of distinct columns, a plan each, for a result
//               that reads both columns of a pair in one round.
//   hub cut     gm_col_hub_cut lists the rows of more than C entries and their segments of C; gm_col_hubs_put uploads the lists with a partial buffer.
//   adjacency   k_col_adjacent: the pairs that get a column of their own under the mask flag.
// The walks, their rounds and what a round emits stay with the two files.
#pragma once
#include <algorithm>
#include <unordered_set>
#include <vector>
#include "gm_nbr.h"

#define GM_COL_THREADS 256

struct gm_col_call {
    hipStream_t st;
    int B; int32_t C;             // the knobs in force
    gm_nbr_graph G;
};

// the two knobs of a call as gm_knob() holds them, their printed names, the bound of `cols` and the library's choices (a knob of 0)
struct gm_col_knobs {
    int cols; const char* cols_name; int chunk; const char* chunk_name;
    int max_cols, cols_default; int32_t chunk_default;
};

// what the calls check behind their own parameters (gm_store_call_check comes first), then the call's frame; n == 0 leaves c->B == 0 (nothing to do)
static inline int gm_col_setup(const char* what, const gm_col_knobs& K, const gm_store* s, int32_t g, int64_t n, const void* d_in, const void* d_out, void* stream, gm_col_call* c) {
    GM_REQUIRE(K.cols >= 0 && K.cols % GM_WAVE == 0 && K.cols <= K.max_cols, GM_EINVAL, "%s: %s = %d; a multiple of 64 up to %d (0: the library's choice)", what, K.cols_name, K.cols,
               K.max_cols);
    GM_REQUIRE(K.chunk >= 0, GM_EINVAL, "%s: %s = %d", what, K.chunk_name, K.chunk);
    c->B = 0;
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_in && d_out, GM_EINVAL, "%s: NULL argument", what);
    GM_TRY(gm_nbr_index(s));
    *c = {(hipStream_t)stream, K.cols ? K.cols : K.cols_default, K.chunk ? K.chunk : K.chunk_default, gm_nbr_graph_of(s, g)};
    return GM_OK;
}

// adj[k] = 1 where the two nodes of pair k are distinct, inside the graph and neighbours (the pairs whose masked columns differ from the unmasked ones).
// static: the translation units are built without relocatable device code, each one that includes this header launches a copy of its own
static __global__ void __launch_bounds__(GM_COL_THREADS) k_col_adjacent(gm_nbr_graph G, const int32_t* __restrict__ pairs, int64_t n, uint8_t* __restrict__ adj) {
    const int64_t k = (int64_t)blockIdx.x * GM_COL_THREADS + threadIdx.x;
    if (k >= n) return;
    adj[k] = gm_nbr_adjacent(G, pairs[2 * k], pairs[2 * k + 1]) ? 1 : 0;
}

// want[e]: the column of output entry e as gm_col_key packs it, -1: no column (a node outside the graph).  -> cs / cx: the distinct columns in ascending
// (source, excluded) order; order: the entries stably by column number, those without a column first; col[i]: the column number of entry order[i] (-1: none).
// h_ptr: the graph's row pointers on the host, for the hub cut (gm_col_sources / gm_col_pairs; pinned memory of the call's stager)
struct gm_col_plan {
    std::vector<int32_t> cs, cx, col;
    std::vector<int64_t> order;
    const int64_t* h_ptr = nullptr;
};
static inline int64_t gm_col_key(int32_t src, int32_t x) { return ((int64_t)src << 32) | (uint32_t)(x + 1); }
static inline int gm_col_plan_of(const char* what, const std::vector<int64_t>& want, gm_col_plan* P) {
    std::vector<int64_t> keys;
    for (const int64_t w : want)
        if (w >= 0) keys.push_back(w);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    GM_REQUIRE(keys.size() <= (size_t)INT32_MAX, GM_ERANGE, "%s: %lld distinct columns", what, (long long)keys.size());
    P->cs.resize(keys.size()); P->cx.resize(keys.size());
    for (size_t k = 0; k < keys.size(); ++k) { P->cs[k] = (int32_t)(keys[k] >> 32); P->cx[k] = (int32_t)(uint32_t)keys[k] - 1; }
    std::vector<int32_t> ecol(want.size());
    for (size_t e = 0; e < want.size(); ++e) ecol[e] = want[e] < 0 ? -1 : (int32_t)(std::lower_bound(keys.begin(), keys.end(), want[e]) - keys.begin());
    P->order.resize(want.size());
    for (size_t e = 0; e < want.size(); ++e) P->order[e] = (int64_t)e;
    std::stable_sort(P->order.begin(), P->order.end(), [&](int64_t p, int64_t q) { return ecol[(size_t)p] < ecol[(size_t)q]; });
    P->col.resize(want.size());
    for (size_t e = 0; e < want.size(); ++e) P->col[e] = ecol[(size_t)P->order[e]];
    return GM_OK;
}

// [lo, hi) of the ascending column numbers `col` that a round starting at column c0 serves: its own columns, and with `none` in the first round the -1s (no column)
static inline void gm_col_span(const std::vector<int32_t>& col, int64_t c0, int64_t Br, bool none, int64_t* lo, int64_t* hi) {
    *lo = none && c0 == 0 ? 0 : std::lower_bound(col.begin(), col.end(), c0) - col.begin();
    *hi = std::lower_bound(col.begin(), col.end(), c0 + Br) - col.begin();
}

// The plan of m sources, one entry per output row: the whole-graph column of its source.  Reads the sources and the row pointers back (ONE synchronisation of
// the stream: what the caller enqueued before, such as a prefill of its output, is complete behind it) -> d_row[i]: the output row of entry i, d_col = P->col
static inline int gm_col_sources(const char* what, const gm_col_call& c, const int32_t* d_sources, int64_t m, gm_stager& sg, gm_scratch& sc, gm_col_plan* P, int32_t** d_row,
                                 int32_t** d_col) {
    const int64_t N = c.G.N;
    const int32_t* h_src = sg.download(d_sources, (size_t)m);
    P->h_ptr = sg.download(c.G.ptr, (size_t)(N + 1));
    GM_REQUIRE(h_src && P->h_ptr, GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(c.st));
    std::vector<int64_t> want((size_t)m, -1);
    for (int64_t r = 0; r < m; ++r)
        if (h_src[r] >= 0 && h_src[r] < N) want[(size_t)r] = gm_col_key(h_src[r], -1);
    GM_TRY(gm_col_plan_of(what, want, P));
    const std::vector<int32_t> row(P->order.begin(), P->order.end());      // (m <= INT32_MAX output rows: gm_store_call_check)
    GM_TRY(sc.put(d_row, row, sg));
    return sc.put(d_col, P->col, sg);
}

// A call's n pairs, with `mask` their adjacency bytes (k_col_adjacent; else NULL), and the graph's row pointers, read back into pinned memory of the call's
// stager behind ONE synchronisation of the stream, as gm_col_sources reads
struct gm_col_pairs_host { const int32_t* pairs = nullptr; const uint8_t* adj = nullptr; const int64_t* ptr = nullptr; };
static inline int gm_col_pairs_read(const char* what, const gm_col_call& c, const int32_t* d_pairs, int64_t n, bool mask, gm_stager& sg, gm_scratch& sc, gm_col_pairs_host* R) {
    uint8_t* d_adj = nullptr;
    if (mask) {
        GM_TRY(sc.take(&d_adj, (size_t)n));
        hipLaunchKernelGGL(k_col_adjacent, dim3((unsigned)((n + GM_COL_THREADS - 1) / GM_COL_THREADS)), dim3(GM_COL_THREADS), 0, c.st, c.G, d_pairs, n, d_adj);
        GM_HIP(hipGetLastError());
        R->adj = sg.download((const uint8_t*)d_adj, (size_t)n);
    }
    R->pairs = sg.download(d_pairs, (size_t)2 * (size_t)n);
    R->ptr = sg.download(c.G.ptr, (size_t)(c.G.N + 1));
    GM_REQUIRE(R->pairs && R->ptr && (!mask || R->adj), GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(c.st));
    return GM_OK;
}

// The plan of n pairs, canonicalised to (u, v) = (min, max); x = the other endpoint for an adjacent pair under `mask`, else -1.  With `both`, entry 2k is
// (u, x)[v] and entry 2k + 1 is (v, x')[u]; without, entry k is (u, x)[v]; a pair with a node outside the graph has no column.  Reads back as gm_col_sources
// does, the adjacency bytes (k_col_adjacent) first -> d_dst = P->order: where entry i goes, d_node[i]: the node it reads in its column, d_col = P->col
static inline int gm_col_pairs(const char* what, const gm_col_call& c, const int32_t* d_pairs, int64_t n, bool mask, bool both, gm_stager& sg, gm_scratch& sc, gm_col_plan* P,
                               int64_t** d_dst, int32_t** d_node, int32_t** d_col) {
    const int64_t N = c.G.N;
    gm_col_pairs_host R;
    GM_TRY(gm_col_pairs_read(what, c, d_pairs, n, mask, sg, sc, &R));
    const int32_t* h_pairs = R.pairs;
    const uint8_t* h_adj = R.adj;
    P->h_ptr = R.ptr;
    const size_t per = both ? 2 : 1;
    std::vector<int64_t> want(per * (size_t)n, -1);
    std::vector<int32_t> node(per * (size_t)n, 0);
    for (int64_t k = 0; k < n; ++k) {
        const int32_t p = h_pairs[2 * k], q = h_pairs[2 * k + 1];
        if (p < 0 || p >= N || q < 0 || q >= N) continue;
        const int32_t u = p < q ? p : q, v = p < q ? q : p;
        const bool cut = mask && h_adj[k];
        const size_t e = per * (size_t)k;
        want[e] = gm_col_key(u, cut ? v : -1); node[e] = v;
        if (both) { want[e + 1] = gm_col_key(v, cut ? u : -1); node[e + 1] = u; }
    }
    GM_TRY(gm_col_plan_of(what, want, P));
    std::vector<int32_t> nd(node.size());
    for (size_t e = 0; e < nd.size(); ++e) nd[e] = node[(size_t)P->order[e]];
    GM_TRY(sc.put(d_dst, P->order, sg)); GM_TRY(sc.put(d_node, nd, sg));
    return sc.put(d_col, P->col, sg);
}

// The pairs of a call whose result needs BOTH columns of a pair, (u, x) and (v, x'), alive in the same round: the canonical pairs sorted by (u, v) and cut
// greedily into groups of at most B DISTINCT columns each (a pair brings at most two, so any B >= 2 holds every pair).  A group is a plan of its own
// (plan: its columns, ascending) and the entries [first, first + cnt) of the lists: pair dst[i] of the call reads the columns cu[i], cv[i] of its group's plan.
// A pair with a node outside the graph is in no group.
struct gm_col_group { gm_col_plan plan; int64_t first = 0, cnt = 0; };
struct gm_col_groups {
    std::vector<gm_col_group> groups;
    std::vector<int64_t> dst;
    std::vector<int32_t> cu, cv;
};
static inline int gm_col_pair_groups(const char* what, int64_t N, const gm_col_pairs_host& R, int64_t n, bool mask, int64_t B, gm_col_groups* G) {
    struct item { int32_t u, v; int64_t k; };
    std::vector<item> items;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t p = R.pairs[2 * k], q = R.pairs[2 * k + 1];
        if (p < 0 || p >= N || q < 0 || q >= N) continue;
        items.push_back({p < q ? p : q, p < q ? q : p, k});
    }
    std::stable_sort(items.begin(), items.end(), [](const item& a, const item& b) { return a.u != b.u ? a.u < b.u : a.v < b.v; });
    G->dst.resize(items.size()); G->cu.resize(items.size()); G->cv.resize(items.size());
    std::unordered_set<int64_t> held;                                          // the distinct columns of the open group
    std::vector<int64_t> want;                                                 // ... and its entries: two per pair
    size_t first = 0;
    const auto close = [&](size_t end) -> int {
        if (end == first) return GM_OK;
        G->groups.emplace_back();
        gm_col_group& g = G->groups.back();
        g.first = (int64_t)first; g.cnt = (int64_t)(end - first); g.plan.h_ptr = R.ptr;
        GM_TRY(gm_col_plan_of(what, want, &g.plan));
        for (size_t e = 0; e < want.size(); ++e) {                             // entry order[e] = 2 i (the u side) or 2 i + 1 (the v side) of the group's pair i
            const size_t at = first + (size_t)(g.plan.order[e] >> 1);
            (g.plan.order[e] & 1 ? G->cv : G->cu)[at] = g.plan.col[e];
        }
        held.clear(); want.clear(); first = end;
        return GM_OK;
    };
    for (size_t i = 0; i < items.size(); ++i) {
        const item& it = items[i];
        const bool cut = mask && R.adj[it.k];
        const int64_t ku = gm_col_key(it.u, cut ? it.v : -1), kv = gm_col_key(it.v, cut ? it.u : -1);
        const int64_t fresh = (held.count(ku) ? 0 : 1) + (kv != ku && !held.count(kv) ? 1 : 0);
        if ((int64_t)held.size() + fresh > B) GM_TRY(close(i));
        held.insert(ku); held.insert(kv);
        want.push_back(ku); want.push_back(kv);
        G->dst[i] = it.k;
    }
    return close(items.size());
}

// The hub rows of the cut at C entries and their segments.  Host: row[h] the h-th hub row, first[h] its first item (first[n_hubs]: the number of items),
// item i = segment it_seg[i] of row it_row[i].  Device (gm_col_hubs_put): the same lists and part[n_items, width], a partial result per segment
struct gm_col_hub_lists { std::vector<int32_t> row, first, it_row, it_seg; };
template <class T>
struct gm_col_hubs {
    int64_t n_hubs = 0, n_items = 0;
    int32_t *row = nullptr, *first = nullptr, *it_row = nullptr, *it_seg = nullptr;
    T* part = nullptr;
};
// at most 2^seg_bits - 1 segments (what the caller's launches over segments can index); chunk_name: the knob behind C as the message prints it
static inline int gm_col_hub_cut(const char* what, const int64_t* h_ptr, int64_t N, int32_t C, int seg_bits, const char* chunk_name, gm_col_hub_lists* L) {
    for (int64_t v = 0; v < N; ++v) {
        const int64_t deg = h_ptr[v + 1] - h_ptr[v];
        if (deg <= C) continue;
        L->row.push_back((int32_t)v); L->first.push_back((int32_t)L->it_row.size());
        for (int64_t seg = 0; seg * C < deg; ++seg) { L->it_row.push_back((int32_t)v); L->it_seg.push_back((int32_t)seg); }
        GM_REQUIRE(L->it_row.size() < ((size_t)1 << seg_bits), GM_ERANGE, "%s: more than 2^%d hub segments at %s = %d", what, seg_bits, chunk_name, (int)C);
    }
    L->first.push_back((int32_t)L->it_row.size());
    return GM_OK;
}
template <class T>
static inline int gm_col_hubs_put(gm_col_hubs<T>* H, const gm_col_hub_lists& L, int64_t width, gm_scratch& sc, gm_stager& sg) {
    H->n_hubs = (int64_t)L.row.size(); H->n_items = (int64_t)L.it_row.size();
    if (!H->n_hubs) return GM_OK;
    GM_TRY(sc.take(&H->part, (size_t)(H->n_items * width)));
    GM_TRY(sc.put(&H->row, L.row, sg)); GM_TRY(sc.put(&H->first, L.first, sg));
    GM_TRY(sc.put(&H->it_row, L.it_row, sg));
    return sc.put(&H->it_seg, L.it_seg, sg);
}
