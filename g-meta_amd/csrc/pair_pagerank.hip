// Rooted PageRank of sources and node pairs (gm_store_rooted_pagerank, gm_store_pair_pagerank: the one global score among the link-prediction baselines).
// The DEFINITION is in include/gmeta_hip.h; tests/pagerank_ref.py restates it in float64.  This file is how it is computed, over the neighbour index
// (nbr_index.hip; gm_nbr.h):
//   columns     a column is a pair (s, x): the walk from s in the graph without the edge {s, x} (x = -1: the whole graph).  The host reads the sources or pairs
//               back once, forms the DISTINCT columns in ascending (s, x) order and runs them in rounds of at most B (gm_set_tuning("ppr_cols")); with the mask
//               flag only adjacent pairs get a column of their own.  The call's frame -- knob checks, read-back and plan, adjacency, hub cut -- is gm_columns.h.
//   the state   Q[N, B] fp32, row-major: p_t[z] / deg' z, pre-scaled per column (a row without neighbours keeps p_t[z] itself), so that a step of the walk is
//               one load and one add per neighbour.  Two buffers swap between iterations; the last iteration stores p itself.
//   one row     a wave takes a row v and a slab of 64 columns: lanes are columns, the neighbour id is wave-uniform (scalar loads), and every neighbour costs one
//               coalesced 256-byte row read of Q -- the gathered whole-row pattern.  GM_PPR_UNROLL row reads are in flight per lane; the adds follow in
//               ascending neighbour order.  The mask is per lane: one excluded id on the two rows v in {s, x} (its term is replaced by +0, which changes no
//               bit) and a degree one less when those two rows are scaled.
//   hub rows    a row of more than C entries (gm_set_tuning("ppr_chunk")) is cut into segments of C: k_ppr_parts sums each segment into a partial buffer
//               (a wave per segment and slab), k_ppr_hubs adds the partials in ascending segment order and finishes the row.  Plain vector stores.
//   results     gm_store_rooted_pagerank: k_ppr_rows_out transposes p[N, B] into the rows of d_out through a 64 x 64 LDS tile (a column serves every duplicate
//               of its source); gm_store_pair_pagerank: k_ppr_entries_out gathers the two wanted entries of every pair; gm_store_pagerank_candidates:
//               the top k of every column, selected on p[N, B] where it lies (gm_pprc_round, pagerank_candidates.hip), so that only [m, k] is written.
// No float atomics, nothing depends on arrival order: a column's bits are a function of (graph, s, x, alpha, iters, C) alone.  Everything runs on the caller's
// stream; scratch comes from the stream-ordered pool.
#include <math.h>
#include "gm_columns.h"

#define GM_PPR_THREADS 256
#define GM_PPR_WAVES (GM_PPR_THREADS / GM_WAVE)
#define GM_PPR_UNROLL 8                   // row reads of Q in flight per lane
#define GM_PPR_TILE 64                    // k_ppr_rows_out: nodes x output rows per workgroup
#define GM_PPR_MAX_COLS 4096

// the columns of one round: source and excluded node per column (-1: no column / no excluded node), B a multiple of 64
struct ppr_cols {
    const int32_t* s; const int32_t* x;
    int32_t B;
};

// the lane's column on the row v: its source and the id the row must skip (-1: none; >= 0 exactly when v is an endpoint of the column's removed edge)
template <bool MASK>
__device__ __forceinline__ void ppr_lane(const ppr_cols& K, int32_t c, int32_t v, int32_t* cs, int32_t* ex) {
    *cs = K.s[c]; *ex = -1;
    if (MASK) { const int32_t cx = K.x[c]; *ex = cx < 0 ? -1 : v == *cs ? cx : v == cx ? *cs : -1; }
}

// sum over row[0 .. len) of Q[z, c] in ascending order (Qc = Q + c); the excluded id's term is +0
template <bool MASK>
__device__ __forceinline__ float ppr_sum(const int32_t* __restrict__ row, int32_t len, const float* __restrict__ Qc, int64_t B, int32_t ex) {
    float acc = 0.f;
    int32_t i = 0;
    for (; i + GM_PPR_UNROLL <= len; i += GM_PPR_UNROLL) {
        int32_t z[GM_PPR_UNROLL]; float q[GM_PPR_UNROLL];
#pragma unroll
        for (int k = 0; k < GM_PPR_UNROLL; ++k) z[k] = row[i + k];
#pragma unroll
        for (int k = 0; k < GM_PPR_UNROLL; ++k) q[k] = Qc[(int64_t)z[k] * B];
#pragma unroll
        for (int k = 0; k < GM_PPR_UNROLL; ++k) acc = __fadd_rn(acc, MASK && z[k] == ex ? 0.f : q[k]);
    }
    for (; i < len; ++i) {
        const int32_t z = row[i];
        const float q = Qc[(int64_t)z * B];
        acc = __fadd_rn(acc, MASK && z == ex ? 0.f : q);
    }
    return acc;
}

// p_{t+1}[v] of the lane's column from the row sum, stored pre-scaled for the next iteration (the last one stores p itself)
__device__ __forceinline__ void ppr_store(float sum, int32_t deg, int32_t v, int32_t cs, int32_t ex, float a, float b, int last, const float* __restrict__ Qa,
                                          float* __restrict__ Qb, int64_t at) {
    const int32_t d = deg - (ex >= 0 ? 1 : 0);                                // deg' v
    const float m = d > 0 ? sum : Qa[at];                                    // a node without neighbours keeps its mass (its Q entry is p itself)
    const float p = __fadd_rn(v == cs ? a : 0.f, __fmul_rn(b, m));
    Qb[at] = last || d == 0 ? p : __fmul_rn(p, __fdiv_rn(1.f, (float)d));
}

// p_0 = e_s, pre-scaled: one thread per column (Q is zero beforehand)
__global__ void __launch_bounds__(GM_PPR_THREADS) k_ppr_seed(gm_nbr_graph G, ppr_cols K, float* __restrict__ Q) {
    const int32_t c = (int32_t)(blockIdx.x * GM_PPR_THREADS + threadIdx.x);
    if (c >= K.B) return;
    const int32_t cs = K.s[c];
    if (cs < 0 || cs >= G.N) return;
    const int32_t d = (int32_t)(G.ptr[cs + 1] - G.ptr[cs]) - (K.x[c] >= 0 ? 1 : 0);
    Q[(int64_t)cs * K.B + c] = d > 0 ? __fdiv_rn(1.f, (float)d) : 1.f;
}

// a wave per (row, slab of 64 columns); rows of more than C entries are left to k_ppr_parts / k_ppr_hubs
template <bool MASK>
__global__ void __launch_bounds__(GM_PPR_THREADS) k_ppr_rows(gm_nbr_graph G, ppr_cols K, int32_t slabs, int32_t C, float a, float b, int last,
                                                             const float* __restrict__ Qa, float* __restrict__ Qb) {
    const int64_t w = (int64_t)blockIdx.x * GM_PPR_WAVES + (threadIdx.x >> 6);
    const int64_t row = w / slabs;
    if (row >= G.N) return;
    const int32_t v = __builtin_amdgcn_readfirstlane((int32_t)row);
    const int32_t slab = __builtin_amdgcn_readfirstlane((int32_t)(w - row * slabs));
    const int32_t c = slab * GM_WAVE + ((int32_t)threadIdx.x & (GM_WAVE - 1));
    const int64_t r0 = G.ptr[v];
    const int32_t deg = (int32_t)(G.ptr[v + 1] - r0);
    if (deg > C) return;
    int32_t cs, ex;
    ppr_lane<MASK>(K, c, v, &cs, &ex);
    const float sum = ppr_sum<MASK>(G.idx + r0, deg, Qa + c, K.B, ex);
    ppr_store(sum, deg, v, cs, ex, a, b, last, Qa, Qb, (int64_t)v * K.B + c);
}

// a wave per (segment of a hub row, slab): part[item, c] = the segment's sum
template <bool MASK>
__global__ void __launch_bounds__(GM_PPR_THREADS) k_ppr_parts(gm_nbr_graph G, ppr_cols K, int32_t slabs, int32_t C, const int32_t* __restrict__ it_row,
                                                              const int32_t* __restrict__ it_seg, int64_t n_items, const float* __restrict__ Qa, float* __restrict__ part) {
    const int64_t w = (int64_t)blockIdx.x * GM_PPR_WAVES + (threadIdx.x >> 6);
    const int64_t item = w / slabs;
    if (item >= n_items) return;
    const int32_t it = __builtin_amdgcn_readfirstlane((int32_t)item);
    const int32_t slab = __builtin_amdgcn_readfirstlane((int32_t)(w - item * slabs));
    const int32_t c = slab * GM_WAVE + ((int32_t)threadIdx.x & (GM_WAVE - 1));
    const int32_t v = it_row[it];
    const int64_t r0 = G.ptr[v], beg = (int64_t)it_seg[it] * C;
    const int64_t left = G.ptr[v + 1] - r0 - beg;
    const int32_t len = (int32_t)(left < C ? left : C);
    int32_t cs, ex;
    ppr_lane<MASK>(K, c, v, &cs, &ex);
    part[(int64_t)it * K.B + c] = ppr_sum<MASK>(G.idx + r0 + beg, len, Qa + c, K.B, ex);
}

// a wave per (hub row, slab): its partials in ascending segment order, then the row as k_ppr_rows finishes it
template <bool MASK>
__global__ void __launch_bounds__(GM_PPR_THREADS) k_ppr_hubs(gm_nbr_graph G, ppr_cols K, int32_t slabs, const int32_t* __restrict__ hub_row,
                                                             const int32_t* __restrict__ hub_first, int64_t n_hubs, float a, float b, int last,
                                                             const float* __restrict__ part, const float* __restrict__ Qa, float* __restrict__ Qb) {
    const int64_t w = (int64_t)blockIdx.x * GM_PPR_WAVES + (threadIdx.x >> 6);
    const int64_t hub = w / slabs;
    if (hub >= n_hubs) return;
    const int32_t h = __builtin_amdgcn_readfirstlane((int32_t)hub);
    const int32_t slab = __builtin_amdgcn_readfirstlane((int32_t)(w - hub * slabs));
    const int32_t c = slab * GM_WAVE + ((int32_t)threadIdx.x & (GM_WAVE - 1));
    const int32_t v = hub_row[h], first = hub_first[h], segs = hub_first[h + 1] - first;
    const int32_t deg = (int32_t)(G.ptr[v + 1] - G.ptr[v]);
    int32_t cs, ex;
    ppr_lane<MASK>(K, c, v, &cs, &ex);
    float sum = part[(int64_t)first * K.B + c];
    for (int32_t k = 1; k < segs; ++k) sum = __fadd_rn(sum, part[(int64_t)(first + k) * K.B + c]);
    ppr_store(sum, deg, v, cs, ex, a, b, last, Qa, Qb, (int64_t)v * K.B + c);
}

// gm_store_rooted_pagerank: out[row[r], v] = P[v, col[r] - c0] for the cnt output rows of a round (col < 0: a source outside the graph, a row of zeros), a
// 64 x 64 tile per workgroup through LDS so that both sides move whole 256-byte pieces
__global__ void __launch_bounds__(GM_PPR_THREADS) k_ppr_rows_out(const float* __restrict__ P, int32_t B, int64_t c0, int64_t N, const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                                 int64_t cnt, int64_t v_tiles, float* __restrict__ out) {
    __shared__ float tile[GM_PPR_TILE][GM_PPR_TILE + 1];
    const int64_t v0 = ((int64_t)blockIdx.x % v_tiles) * GM_PPR_TILE, r0 = ((int64_t)blockIdx.x / v_tiles) * GM_PPR_TILE;
    const int hi = (int)threadIdx.x >> 6, lo = (int)threadIdx.x & 63;
    {
        const int64_t r = r0 + lo;
        const int64_t c = r < cnt ? (int64_t)col[r] - c0 : -1;                       // (a round's first column is c0; -1 stays negative)
        for (int i = 0; i < GM_PPR_TILE; i += GM_PPR_WAVES) {
            const int64_t v = v0 + i + hi;
            tile[i + hi][lo] = c >= 0 && v < N ? P[v * B + c] : 0.f;
        }
    }
    __syncthreads();
    const int64_t v = v0 + lo;
    for (int i = 0; i < GM_PPR_TILE; i += GM_PPR_WAVES) {
        const int64_t r = r0 + i + hi;
        if (r < cnt && v < N) out[(int64_t)row[r] * N + v] = tile[lo][i + hi];
    }
}

// gm_store_pair_pagerank: out[dst[e]] = P[node[e], col[e] - c0] for the cnt entries of a round (col < 0: a node outside the graph, zero)
__global__ void __launch_bounds__(GM_PPR_THREADS) k_ppr_entries_out(const float* __restrict__ P, int32_t B, int64_t c0, const int64_t* __restrict__ dst, const int32_t* __restrict__ node,
                                                                    const int32_t* __restrict__ col, int64_t cnt, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * GM_PPR_THREADS + threadIdx.x;
    if (e >= cnt) return;
    const int32_t c = col[e];
    out[dst[e]] = c >= 0 ? P[(int64_t)node[e] * B + (c - c0)] : 0.f;
}

// Columns per round and entries per hub segment, from the sweep at the arxiv shape (profiles/pair_pagerank.txt).  Wider rounds are faster as long as there are
// columns to fill them (1,024 sources: 37.4 / 33.0 / 31.3 ms at 64 / 128 / 256 columns); a round is never wider than the call's columns.  The cut has to be ONE
// value, whatever the round holds: the order of a row sum, hence the bits, belong to it.  Segments of 64 and 256 level everywhere; a round of one slab gains most
// (64 sources: 2.5 ms against 3.9 uncut -- the longest row is the tail of every iteration), a round of four slabs, whose hub rows are spread over four waves
// already, pays the two extra launches per iteration (256 sources: 7.96 ms against 7.48 uncut).  Segments of 1,024 lose on both sides.
static int ppr_cols_for() { return 256; }
static int32_t ppr_chunk_for() { return 256; }

static unsigned ppr_grid(int64_t waves) { return (unsigned)((waves + GM_PPR_WAVES - 1) / GM_PPR_WAVES); }

struct ppr_call : gm_col_call { float alpha; int32_t iters; };

// the checks the exports share; n == 0 leaves c->B == 0 (nothing to do)
static int ppr_begin(const char* what, const char* cnt_name, const gm_store* s, int32_t g, int64_t n, int32_t flags, float alpha, int32_t iters, const void* d_in, const void* d_out,
                     void* stream, ppr_call* c) {
    GM_TRY(gm_store_call_check(what, s, g, cnt_name, n, flags));
    GM_REQUIRE(isfinite(alpha) && alpha > 0.f && alpha < 1.f, GM_EINVAL, "%s: alpha = %g; 0 < alpha < 1", what, (double)alpha);
    GM_REQUIRE(iters >= 1 && iters <= 255, GM_EINVAL, "%s: iters = %d; 1 .. 255", what, iters);
    c->alpha = alpha; c->iters = iters;
    return gm_col_setup(what, {gm_knob().ppr_cols, "ppr_cols", gm_knob().ppr_chunk, "ppr_chunk", GM_PPR_MAX_COLS, ppr_cols_for(), ppr_chunk_for()}, s, g, n, d_in, d_out, stream, c);
}

// one iteration of a round's walk, src -> dst: the rows up to C entries, then the hub rows' segments and the hub rows
template <bool MASK>
static void ppr_iterate(const ppr_call& c, const ppr_cols& K, const gm_col_hubs<float>& H, int last, const float* src, float* dst) {
    const int32_t slabs = K.B / GM_WAVE;
    const float a = c.alpha, b = 1.0f - a;
    const dim3 block(GM_PPR_THREADS), rows(ppr_grid(c.G.N * slabs)), parts(ppr_grid(H.n_items * slabs)), hubs(ppr_grid(H.n_hubs * slabs));
    hipLaunchKernelGGL(k_ppr_rows<MASK>, rows, block, 0, c.st, c.G, K, slabs, c.C, a, b, last, src, dst);
    if (!H.n_hubs) return;
    hipLaunchKernelGGL(k_ppr_parts<MASK>, parts, block, 0, c.st, c.G, K, slabs, c.C, (const int32_t*)H.it_row, (const int32_t*)H.it_seg, H.n_items, src, H.part);
    hipLaunchKernelGGL(k_ppr_hubs<MASK>, hubs, block, 0, c.st, c.G, K, slabs, (const int32_t*)H.row, (const int32_t*)H.first, H.n_hubs, a, b, last, (const float*)H.part, src, dst);
}

// The walk of the plan's columns (cs[k], cx[k]), ascending, in rounds of at most B: after a round's last iteration emit(c0, Br, P) reads P[N, Br] = p of the
// columns c0 .. c0 + Br on the call's stream (Br == 0, P == NULL: a call without a single column); P is the round's scratch, dead behind the emit, which may
// write to it.
template <class Emit>
static int ppr_rounds(const char* what, const ppr_call& c, const gm_col_plan& pl, gm_stager& sg, Emit emit) {
    const gm_nbr_graph& G = c.G;
    std::vector<int32_t> cs(pl.cs), cx(pl.cx);
    const int64_t N = G.N, ncols = (int64_t)cs.size(), ncp = (ncols + GM_WAVE - 1) / GM_WAVE * GM_WAVE;
    cs.resize((size_t)ncp, -1); cx.resize((size_t)ncp, -1);
    const int64_t Bmax = ncp < c.B ? ncp : c.B;
    GM_REQUIRE(N * (Bmax / GM_WAVE + 1) <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld nodes x %lld columns per round pass the launch's 2^31 waves", what, (long long)N, (long long)Bmax);
    gm_col_hub_lists hl;
    GM_TRY(gm_col_hub_cut(what, pl.h_ptr, N, c.C, 30, "ppr_chunk", &hl));      // (INT32_MAX / 2 segments)
    gm_col_hubs<float> H;

    gm_scratch sc(c.st);
    float *Qa = nullptr, *Qb = nullptr;
    int32_t *d_cs = nullptr, *d_cx = nullptr;
    if (ncols) {
        GM_TRY(sc.take(&Qa, (size_t)(N * Bmax))); GM_TRY(sc.take(&Qb, (size_t)(N * Bmax)));
        GM_TRY(sc.put(&d_cs, cs, sg)); GM_TRY(sc.put(&d_cx, cx, sg));
        GM_TRY(gm_col_hubs_put(&H, hl, Bmax, sc, sg));
    }
    for (int64_t c0 = 0; c0 == 0 || c0 < ncp; c0 += c.B) {
        const int32_t Br = (int32_t)(ncp - c0 < c.B ? ncp - c0 : c.B);
        float* P = nullptr;                                                        // (scratch: an emit may overwrite it)
        if (Br) {
            const ppr_cols K = {d_cs + c0, d_cx + c0, Br};
            bool mask = false;
            for (int32_t k = 0; k < Br && !mask; ++k) mask = cx[(size_t)(c0 + k)] >= 0;
            GM_HIP(hipMemsetAsync(Qa, 0, (size_t)(N * Br) * sizeof(float), c.st));
            hipLaunchKernelGGL(k_ppr_seed, dim3((unsigned)((Br + GM_PPR_THREADS - 1) / GM_PPR_THREADS)), dim3(GM_PPR_THREADS), 0, c.st, G, K, Qa);
            float *src = Qa, *dst = Qb;
            for (int32_t t = 0; t < c.iters; ++t) {
                (mask ? ppr_iterate<true> : ppr_iterate<false>)(c, K, H, t == c.iters - 1, src, dst);
                GM_HIP(hipGetLastError());
                std::swap(src, dst);
            }
            P = src;
        }
        GM_TRY(emit(c0, Br, P));
    }
    return GM_OK;
}

extern "C" int32_t gm_store_rooted_pagerank(const gm_store_t* s, int32_t g, const int32_t* d_sources, int64_t m, float alpha, int32_t iters, float* d_out, void* stream) {
    const char* what = "gm_store_rooted_pagerank";
    ppr_call c;
    GM_TRY(ppr_begin(what, "m", s, g, m, 0, alpha, iters, d_sources, d_out, stream, &c));
    if (!c.B) return GM_OK;
    const int64_t N = c.G.N;
    gm_stager sg(c.st);
    gm_scratch sc(c.st);
    gm_col_plan pl;
    int32_t *d_row = nullptr, *d_col = nullptr;
    GM_TRY(gm_col_sources(what, c, d_sources, m, sg, sc, &pl, &d_row, &d_col));
    const int64_t v_tiles = (N + GM_PPR_TILE - 1) / GM_PPR_TILE;
    return ppr_rounds(what, c, pl, sg, [&](int64_t c0, int32_t Br, const float* P) {
        int64_t lo, hi;
        gm_col_span(pl.col, c0, Br, true, &lo, &hi);
        if (hi == lo) return (int)GM_OK;
        const int64_t blocks = v_tiles * ((hi - lo + GM_PPR_TILE - 1) / GM_PPR_TILE);
        GM_REQUIRE(blocks <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld output tiles in one round", what, (long long)blocks);
        hipLaunchKernelGGL(k_ppr_rows_out, dim3((unsigned)blocks), dim3(GM_PPR_THREADS), 0, c.st, P, Br, c0, N, (const int32_t*)d_row + lo, (const int32_t*)d_col + lo, hi - lo,
                           v_tiles, d_out);
        GM_HIP(hipGetLastError());
        return (int)GM_OK;
    });
}

extern "C" int32_t gm_store_pair_pagerank(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, float alpha, int32_t iters, float* d_out, void* stream) {
    const char* what = "gm_store_pair_pagerank";
    ppr_call c;
    GM_TRY(ppr_begin(what, "n", s, g, n, flags, alpha, iters, d_pairs, d_out, stream, &c));
    if (!c.B) return GM_OK;
    gm_scratch sc(c.st);
    gm_stager sg(c.st);
    gm_col_plan pl;                                                        // two entries per pair: pi of v from u, pi of u from v
    int64_t* d_dst = nullptr;
    int32_t *d_node = nullptr, *d_col = nullptr;
    GM_TRY(gm_col_pairs(what, c, d_pairs, n, (flags & GM_PAIR_MASK_TARGET) != 0, true, sg, sc, &pl, &d_dst, &d_node, &d_col));
    return ppr_rounds(what, c, pl, sg, [&](int64_t c0, int32_t Br, const float* P) {
        int64_t lo, hi;
        gm_col_span(pl.col, c0, Br, true, &lo, &hi);
        if (hi == lo) return (int)GM_OK;
        hipLaunchKernelGGL(k_ppr_entries_out, dim3((unsigned)((hi - lo + GM_PPR_THREADS - 1) / GM_PPR_THREADS)), dim3(GM_PPR_THREADS), 0, c.st, P, Br, c0,
                           (const int64_t*)d_dst + lo, (const int32_t*)d_node + lo, (const int32_t*)d_col + lo, hi - lo, d_out);
        GM_HIP(hipGetLastError());
        return (int)GM_OK;
    });
}

// The top k of every source's row, selected on the round's state while it is in scratch (pagerank_candidates.hip): the rows, columns and rounds are those of
// gm_store_rooted_pagerank, so the scores are its bits
extern "C" int32_t gm_store_pagerank_candidates(const gm_store_t* s, int32_t g, const int32_t* d_nodes, int64_t m, int32_t k, float alpha, int32_t iters, int32_t* d_out_nodes,
                                                float* d_out_scores, int32_t* d_out_total, void* stream) {
    const char* what = "gm_store_pagerank_candidates";
    ppr_call c;
    GM_TRY(ppr_begin(what, "m", s, g, m, 0, alpha, iters, d_nodes, d_out_nodes, stream, &c));
    GM_REQUIRE(k >= 1 && k <= GM_CAND_MAX_K, GM_EINVAL, "%s: k = %d; 1 .. %d", what, k, GM_CAND_MAX_K);
    if (!c.B) return GM_OK;
    GM_REQUIRE(d_out_scores && d_out_total, GM_EINVAL, "%s: NULL argument", what);
    gm_phase_timer tm("pagerank candidates");
    const bool timed = gm_knob().timing != 0;
    gm_stager sg(c.st);
    gm_scratch sc(c.st);
    gm_col_plan pl;                                                        // (node ids are int32 in the keys: ppr_rounds holds N below 2^31)
    int32_t *d_row = nullptr, *d_col = nullptr, *d_src = nullptr;
    GM_TRY(gm_col_sources(what, c, d_nodes, m, sg, sc, &pl, &d_row, &d_col));
    const int64_t ncp = ((int64_t)pl.cs.size() + GM_WAVE - 1) / GM_WAVE * GM_WAVE;
    std::vector<int32_t> src(pl.cs);
    src.resize((size_t)ncp, -1);                                           // (as ppr_rounds pads its columns)
    GM_TRY(sc.put(&d_src, src, sg));
    gm_pprc sel;
    GM_TRY(gm_pprc_prepare(&sel, sc, (int32_t)(ncp < c.B ? ncp : c.B), k, c.st));
    if (timed) { GM_HIP(hipStreamSynchronize(c.st)); tm.lap("plan"); }
    return ppr_rounds(what, c, pl, sg, [&](int64_t c0, int32_t Br, float* P) {
        int64_t lo, hi;
        gm_col_span(pl.col, c0, Br, true, &lo, &hi);
        return gm_pprc_round(sel, c.G, P, Br, (const int32_t*)d_src + c0, (const int32_t*)d_row + lo, (const int32_t*)d_col + lo, c0, hi - lo, d_out_nodes, d_out_scores,
                             d_out_total, timed ? &tm : nullptr);
    });
}
