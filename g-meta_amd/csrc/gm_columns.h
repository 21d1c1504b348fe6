// The columns of a call that runs one column per (source, excluded node) over the neighbour index, host side: how pair_pagerank.hip and pair_distance.hip form
// the DISTINCT columns of their sources or pairs and the order the output entries leave in.  A column is a pair (s, x): s the source, x = -1 or the node whose
// edge {s, x} the column's graph lacks.
#pragma once
#include <algorithm>
#include <vector>
#include "gm_internal.h"

// want[e]: the column of output entry e as gm_col_key packs it, -1: no column (a node outside the graph).  -> cs / cx: the distinct columns in ascending
// (source, excluded) order; order: the entries stably by column number, those without a column first; col[i]: the column number of entry order[i] (-1: none)
struct gm_col_plan {
    std::vector<int32_t> cs, cx, col;
    std::vector<int64_t> order;
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
