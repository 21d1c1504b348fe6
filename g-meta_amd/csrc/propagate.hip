// BUDDY / SIGN hop-propagated node features of a parent graph (gm_store_propagate_build, gm_prop_*; the DEFINITION is in include/gmeta_hip.h,
// tests/hop_feature_ref.py restates it): x_0 = the store's feature rows, x_{t+1} = A^ x_t with the project's GraphConv normalisation over the WHOLE graph's in-edge
// CSR as the store holds it (parallel edges, self loops, directions and weights kept), optionally with one self loop in front of every row.
//   layout      level-major, then node-major: x[level][node][ld floats], ld = the store's feature row stride (F where F is a multiple of 4, else F padded with
//               zero columns: always a multiple of 4).  Level 0 is STORED (a device copy of the store's rows): the handle holds no pointer into the store.
//   rows        the EXTENDED row of v is its self-loop entry (v, 1.0f) under GM_PROP_SELF_LOOPS, then its in-CSR entries in stored order; entry e of it is CSR
//               entry e - self of the row.  Everything below counts entries of the extended row.
//   norm        k_prop_norm: a thread per row sums the weights in row order (an unweighted row of n entries sums to min(n, 2^24) exactly as n additions of 1.0f
//               do) and stores 1 / sqrtf(d > 0 ? d : 1).  k_prop_coef: a thread per CSR entry forms w_uv * norm(u) ONCE; the levels read it beside the index.
//   a level     k_prop_level<V>: a wave per (row, chunk of 64 V columns), the lanes across the chunk's columns V floats each (V = 4 from ld = 256 on, 2 from
//               128 on, else 1: a full wave where the row is wide enough), so an entry costs one coalesced read of up to 256 V bytes; GM_PR_UNROLL entries'
//               loads are in flight, index and coefficient are wave-uniform scalar loads.  acc = fmaf(c, x, acc) in row order from +0, the row is scaled by
//               norm(v) and stored once.  A column's sum never meets another column: the tiling cannot change a bit.
//   hub rows    rows of more than C entries (gm_set_tuning("prop_chunk"); gm_columns.h: gm_col_hub_cut) are left out of that launch: k_prop_parts sums every
//               segment of C entries from +0 into a partial row in scratch, k_prop_hubs adds a row's partials in ascending order and scales.  The degree sums
//               of hub rows go the same way (k_prop_norm_parts / k_prop_norm_hubs).  No atomics.
//   readers     k_prop_rows / k_prop_pairs: a thread per V output columns, plain gathers with vector stores (V = 4 where F and the output pointer allow).
// A build runs on the caller's stream and is complete on the device when it returns; the levels are read-only afterwards.
#include "gm_columns.h"
#include "gm_devutil.h"

#define GM_PR_THREADS 256
#define GM_PR_WAVES (GM_PR_THREADS / GM_WAVE)
#define GM_PR_UNROLL 8                    // entries' row loads in flight per lane
#define GM_PR_CHUNK 256                   // the library's prop_chunk: entries per segment of a hub row
#define GM_PR_MIB 8192                    // the library's prop_mib: 8 GiB per build
#define GM_PR_MAX_HOPS 8

// (struct gm_prop, the handle, is in gm_internal.h: pair_mlp.hip reads the levels too)
// the in-edge CSR of one graph: ptr = its rows of the store's pointers (GLOBAL edge offsets), idx / w based at the store's edge 0, sources LOCAL to the graph;
// e0 = ptr[0]: coef[e - e0] is the coefficient of edge e
struct pr_graph { const int64_t* ptr; const int32_t* idx; const float* w; int64_t N, e0; int32_t self; };

template <int V> struct alignas(4 * V) pr_vec { float f[V]; };

// acc += c[i] * (V floats at P + idx[i] * ld) over i in [0, len), in that order (idx, c and len wave-uniform)
template <int V>
__device__ __forceinline__ void pr_fold(pr_vec<V>& acc, const int32_t* __restrict__ idx, const float* __restrict__ c, int32_t len, const float* __restrict__ P, int64_t ld) {
    int32_t i = 0;
    for (; i + GM_PR_UNROLL <= len; i += GM_PR_UNROLL) {
        int32_t z[GM_PR_UNROLL]; float a[GM_PR_UNROLL]; pr_vec<V> q[GM_PR_UNROLL];
#pragma unroll
        for (int k = 0; k < GM_PR_UNROLL; ++k) { z[k] = idx[i + k]; a[k] = c[i + k]; }
#pragma unroll
        for (int k = 0; k < GM_PR_UNROLL; ++k) q[k] = *(const pr_vec<V>*)(P + (int64_t)z[k] * ld);
#pragma unroll
        for (int k = 0; k < GM_PR_UNROLL; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) acc.f[j] = __fmaf_rn(a[k], q[k].f[j], acc.f[j]);
    }
    for (; i < len; ++i) {
        const float a = c[i];
        const pr_vec<V> q = *(const pr_vec<V>*)(P + (int64_t)idx[i] * ld);
#pragma unroll
        for (int j = 0; j < V; ++j) acc.f[j] = __fmaf_rn(a, q.f[j], acc.f[j]);
    }
}

// the sum of the entries [beg, end) of the extended row of v, from +0 in row order, at the columns col .. col + V - 1 of `prev`
template <int V>
__device__ __forceinline__ pr_vec<V> pr_segment(const pr_graph& G, int64_t v, int64_t beg, int64_t end, const float* __restrict__ norm, const float* __restrict__ coef,
                                                const float* __restrict__ prev, int64_t ld, int32_t col) {
    pr_vec<V> acc;
#pragma unroll
    for (int j = 0; j < V; ++j) acc.f[j] = 0.f;
    const float* P = prev + col;
    if (G.self && beg == 0) {                                                  // the self loop: (v, 1.0f), coefficient 1.0f * norm(v)
        const float a = norm[v];
        const pr_vec<V> q = *(const pr_vec<V>*)(P + v * ld);
#pragma unroll
        for (int j = 0; j < V; ++j) acc.f[j] = __fmaf_rn(a, q.f[j], acc.f[j]);
    }
    const int64_t r0 = G.ptr[v], lo = r0 + (beg > 0 ? beg - G.self : 0), hi = r0 + end - G.self;
    pr_fold<V>(acc, G.idx + lo, coef + (lo - G.e0), (int32_t)(hi - lo), P, ld);
    return acc;
}

// the wave's work item and its lane's first column: item = blockIdx * waves + wave (wave-uniform), column = V (64 (item % NCH) + lane), clamped into the row so
// that every lane runs the same loads (live: the lane owns its columns)
struct pr_item { int64_t it; int32_t col; bool live; };
template <int V>
__device__ __forceinline__ pr_item pr_item_of(int32_t ld, int32_t NCH) {
    const int32_t lane = (int32_t)threadIdx.x & (GM_WAVE - 1);
    const int32_t w = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x / GM_WAVE);
    const int64_t item = (int64_t)blockIdx.x * GM_PR_WAVES + w;
    const int32_t col = ((int32_t)(item % NCH) * GM_WAVE + lane) * V;
    pr_item r;
    r.it = item / NCH; r.live = col < ld; r.col = r.live ? col : ld - V;
    return r;
}

// ---------------------------------------------------------------------------------------------------- degrees, norms, coefficients
__device__ __forceinline__ float pr_norm_of(float d) { return 1.0f / sqrtf(d > 0.f ? d : 1.0f); }

// the fp32 sum, in row order, of the weights of the entries [beg, end) of the extended row of v
__device__ __forceinline__ float pr_degree(const pr_graph& G, int64_t v, int64_t beg, int64_t end) {
    if (!G.w) { const int64_t n = end - beg; return (float)(n < (1 << 24) ? n : (1 << 24)); }      // n additions of 1.0f stop at 2^24
    float d = G.self && beg == 0 && end > 0 ? 1.0f : 0.f;
    const int64_t r0 = G.ptr[v], lo = r0 + (beg > 0 ? beg - G.self : 0), hi = r0 + end - G.self;
    for (int64_t e = lo; e < hi; ++e) d += G.w[e];
    return d;
}

// norm[v] of the rows of at most C entries.  A thread per row
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_norm(pr_graph G, int32_t C, float* __restrict__ norm) {
    const int64_t v = (int64_t)blockIdx.x * GM_PR_THREADS + threadIdx.x;
    if (v >= G.N) return;
    const int64_t len = G.ptr[v + 1] - G.ptr[v] + G.self;
    if (len > C) return;
    norm[v] = pr_norm_of(pr_degree(G, v, 0, len));
}

// dpart[item] = the degree sum of segment it_seg[item] of hub row it_row[item].  A thread per segment
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_norm_parts(pr_graph G, int32_t C, const int32_t* __restrict__ it_row, const int32_t* __restrict__ it_seg, int64_t n_items,
                                                                   float* __restrict__ dpart) {
    const int64_t it = (int64_t)blockIdx.x * GM_PR_THREADS + threadIdx.x;
    if (it >= n_items) return;
    const int64_t v = it_row[it], len = G.ptr[v + 1] - G.ptr[v] + G.self, beg = (int64_t)it_seg[it] * C;
    dpart[it] = pr_degree(G, v, beg, beg + C < len ? beg + C : len);
}

// norm[v] of a hub row: its segments' sums added in ascending order.  A thread per hub row
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_norm_hubs(const int32_t* __restrict__ hub_row, const int32_t* __restrict__ hub_first, int64_t n_hubs,
                                                                  const float* __restrict__ dpart, float* __restrict__ norm) {
    const int64_t h = (int64_t)blockIdx.x * GM_PR_THREADS + threadIdx.x;
    if (h >= n_hubs) return;
    const int32_t first = hub_first[h], segs = hub_first[h + 1] - first;
    float d = dpart[first];
    for (int32_t k = 1; k < segs; ++k) d += dpart[first + k];
    norm[hub_row[h]] = pr_norm_of(d);
}

// coef[e - e0] = w_uv * norm(u) of CSR entry e.  A thread per entry
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_coef(pr_graph G, int64_t nnz, const float* __restrict__ norm, float* __restrict__ coef) {
    const int64_t k = (int64_t)blockIdx.x * GM_PR_THREADS + threadIdx.x;
    if (k >= nnz) return;
    const int64_t e = G.e0 + k;
    coef[k] = (G.w ? G.w[e] : 1.0f) * norm[G.idx[e]];
}

// ---------------------------------------------------------------------------------------------------- levels
// prev -> next for the rows of at most C entries
template <int V>
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_level(pr_graph G, int32_t C, int32_t ld, int32_t NCH, const float* __restrict__ norm, const float* __restrict__ coef,
                                                              const float* __restrict__ prev, float* __restrict__ next) {
    const pr_item w = pr_item_of<V>(ld, NCH);
    if (w.it >= G.N) return;
    const int64_t len = G.ptr[w.it + 1] - G.ptr[w.it] + G.self;
    if (len > C) return;
    pr_vec<V> acc = pr_segment<V>(G, w.it, 0, len, norm, coef, prev, ld, w.col);
    const float nv = norm[w.it];
#pragma unroll
    for (int j = 0; j < V; ++j) acc.f[j] = nv * acc.f[j];
    if (w.live) *(pr_vec<V>*)(next + w.it * ld + w.col) = acc;
}

// part[item] = the sum of segment it_seg[item] of hub row it_row[item]
template <int V>
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_parts(pr_graph G, int32_t C, int32_t ld, int32_t NCH, const int32_t* __restrict__ it_row, const int32_t* __restrict__ it_seg,
                                                              int64_t n_items, const float* __restrict__ norm, const float* __restrict__ coef, const float* __restrict__ prev,
                                                              float* __restrict__ part) {
    const pr_item w = pr_item_of<V>(ld, NCH);
    if (w.it >= n_items) return;
    const int64_t v = it_row[w.it], len = G.ptr[v + 1] - G.ptr[v] + G.self, beg = (int64_t)it_seg[w.it] * C;
    const pr_vec<V> acc = pr_segment<V>(G, v, beg, beg + C < len ? beg + C : len, norm, coef, prev, ld, w.col);
    if (w.live) *(pr_vec<V>*)(part + w.it * ld + w.col) = acc;
}

// a hub row: its segments' partial rows added in ascending order, scaled by norm(v)
template <int V>
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_hubs(int32_t ld, int32_t NCH, const int32_t* __restrict__ hub_row, const int32_t* __restrict__ hub_first, int64_t n_hubs,
                                                             const float* __restrict__ norm, const float* __restrict__ part, float* __restrict__ next) {
    const pr_item w = pr_item_of<V>(ld, NCH);
    if (w.it >= n_hubs) return;
    const int64_t v = hub_row[w.it];
    const int32_t first = hub_first[w.it], segs = hub_first[w.it + 1] - first;
    pr_vec<V> acc = *(const pr_vec<V>*)(part + (int64_t)first * ld + w.col);
    for (int32_t k = 1; k < segs; ++k) {
        const pr_vec<V> q = *(const pr_vec<V>*)(part + (int64_t)(first + k) * ld + w.col);
#pragma unroll
        for (int j = 0; j < V; ++j) acc.f[j] = acc.f[j] + q.f[j];
    }
    const float nv = norm[v];
#pragma unroll
    for (int j = 0; j < V; ++j) acc.f[j] = nv * acc.f[j];
    if (w.live) *(pr_vec<V>*)(next + v * ld + w.col) = acc;
}

// ---------------------------------------------------------------------------------------------------- readers
// out[i, f] = level[nodes[i], f] (zeros for a node outside the graph), dense [m, F].  A thread per V columns (F a multiple of V)
template <int V>
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_rows(const float* __restrict__ level, int64_t N, int32_t F, int32_t ld, const int32_t* __restrict__ nodes, int64_t m,
                                                             float* __restrict__ out) {
    const int32_t per = F / V;
    const int64_t t = (int64_t)blockIdx.x * GM_PR_THREADS + threadIdx.x;
    if (t >= m * per) return;
    const int64_t i = t / per;
    const int32_t f = (int32_t)(t % per) * V, v = nodes[i];
    pr_vec<V> q;
#pragma unroll
    for (int j = 0; j < V; ++j) q.f[j] = 0.f;
    if (v >= 0 && v < N) q = *(const pr_vec<V>*)(level + (int64_t)v * ld + f);
    *(pr_vec<V>*)(out + i * F + f) = q;
}

// out[k, t, f] = x_t[a][f] * x_t[b][f] (op 0) or |x_t[a][f] - x_t[b][f]| (op 1) of pair k = (a, b); zeros when a node is outside the graph
template <int V>
__global__ void __launch_bounds__(GM_PR_THREADS) k_prop_pairs(const float* __restrict__ x, int64_t N, int32_t L1, int32_t F, int32_t ld, const int32_t* __restrict__ pairs, int64_t n,
                                                              int32_t op, float* __restrict__ out) {
    const int32_t per = F / V;
    const int64_t t = (int64_t)blockIdx.x * GM_PR_THREADS + threadIdx.x;
    if (t >= n * L1 * per) return;
    const int64_t k = t / ((int64_t)L1 * per);
    const int32_t r = (int32_t)(t % ((int64_t)L1 * per)), lv = r / per, f = (r % per) * V;
    const int32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    pr_vec<V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.f[j] = 0.f;
    if (a >= 0 && a < N && b >= 0 && b < N) {
        const float* base = x + (int64_t)lv * N * ld + f;
        const pr_vec<V> qa = *(const pr_vec<V>*)(base + (int64_t)a * ld), qb = *(const pr_vec<V>*)(base + (int64_t)b * ld);
#pragma unroll
        for (int j = 0; j < V; ++j) o.f[j] = op == GM_PROP_HADAMARD ? qa.f[j] * qb.f[j] : fabsf(qa.f[j] - qb.f[j]);
    }
    *(pr_vec<V>*)(out + (k * L1 + lv) * F + f) = o;
}

// ---------------------------------------------------------------------------------------------------- host
static inline unsigned pr_grid(int64_t waves) { return (unsigned)((waves + GM_PR_WAVES - 1) / GM_PR_WAVES); }
static inline unsigned pr_blocks(int64_t threads) { return (unsigned)((threads + GM_PR_THREADS - 1) / GM_PR_THREADS); }

extern "C" void gm_prop_destroy(gm_prop_t* p) {
    if (!p) return;
    if (p->d) (void)hipFree(p->d);                                             // (waits for the device: no kernel still reads the levels)
    delete p;
}

// the H launches of one level width
template <int V>
static int pr_levels(hipStream_t st, const pr_graph& G, int32_t C, const gm_prop* p, const gm_col_hubs<float>& H, const float* norm, const float* coef, gm_phase_timer& tm) {
    const int32_t ld = p->ld, NCH = (ld / V + GM_WAVE - 1) / GM_WAVE;
    const int64_t level = p->N * ld;
    const dim3 block(GM_PR_THREADS);
    for (int32_t t = 1; t <= p->hops; ++t) {
        const float* prev = p->d + (int64_t)(t - 1) * level;
        float* next = p->d + (int64_t)t * level;
        hipLaunchKernelGGL(k_prop_level<V>, dim3(pr_grid(p->N * NCH)), block, 0, st, G, C, ld, NCH, norm, coef, prev, next);
        if (H.n_hubs) {
            hipLaunchKernelGGL(k_prop_parts<V>, dim3(pr_grid(H.n_items * NCH)), block, 0, st, G, C, ld, NCH, (const int32_t*)H.it_row, (const int32_t*)H.it_seg, H.n_items, norm,
                               coef, prev, H.part);
            hipLaunchKernelGGL(k_prop_hubs<V>, dim3(pr_grid(H.n_hubs * NCH)), block, 0, st, ld, NCH, (const int32_t*)H.row, (const int32_t*)H.first, H.n_hubs, norm,
                               (const float*)H.part, next);
        }
        GM_HIP(hipGetLastError());
        if (tm.on) { GM_HIP(hipStreamSynchronize(st)); tm.lap("level"); }
    }
    return GM_OK;
}

extern "C" int32_t gm_store_propagate_build(const gm_store_t* s, int32_t g, int32_t hops, int32_t flags, void* stream, gm_prop_t** out) {
    const char* what = "gm_store_propagate_build";
    GM_TRY(gm_store_call_check(what, s, g));
    GM_REQUIRE(out, GM_EINVAL, "%s: out is NULL", what);
    *out = nullptr;
    GM_REQUIRE(hops >= 1 && hops <= GM_PR_MAX_HOPS, GM_EINVAL, "%s: hops = %d; 1 .. %d", what, hops, GM_PR_MAX_HOPS);
    GM_REQUIRE((flags & ~GM_PROP_SELF_LOOPS) == 0, GM_EINVAL, "%s: unknown flag bits 0x%x (GM_PROP_SELF_LOOPS = 1)", what, (unsigned)flags);
    const int chunk = gm_knob().prop_chunk, mib = gm_knob().prop_mib;
    GM_REQUIRE(chunk >= 0, GM_EINVAL, "%s: prop_chunk = %d", what, chunk);
    GM_REQUIRE(mib >= 0, GM_EINVAL, "%s: prop_mib = %d", what, mib);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t N = s->node_off[g + 1] - s->node_off[g];
    const int32_t ld = s->feat_ld, self = flags & GM_PROP_SELF_LOOPS ? 1 : 0;
    const int64_t level = N * ld, bytes = (int64_t)(hops + 1) * level * (int64_t)sizeof(float), budget = (int64_t)(mib ? mib : GM_PR_MIB) << 20;
    GM_REQUIRE(bytes <= budget, GM_ERANGE, "%s: the levels take %lld bytes at N = %lld, hops = %d, F = %d; prop_mib = %d holds %lld", what, (long long)bytes, (long long)N, hops,
               s->feat_dim, mib ? mib : GM_PR_MIB, (long long)budget);
    GM_REQUIRE((level + GM_PR_WAVES - 1) / GM_PR_WAVES <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld nodes of %d columns pass the launch's 2^31 workgroups", what, (long long)N, ld);
    const int32_t C = chunk ? chunk : GM_PR_CHUNK;

    struct guard { gm_prop* p; ~guard() { gm_prop_destroy(p); } } own = {new gm_prop};
    gm_prop* p = own.p;
    p->N = N; p->bytes = bytes; p->hops = hops; p->F = s->feat_dim; p->ld = ld; p->flags = flags;
    GM_HIP(hipMalloc((void**)&p->d, (size_t)(bytes ? bytes : 4)));
    if (N) {
        gm_stager sg(st);
        gm_scratch sc(st);
        const int64_t* d_ptr = s->d_in_ptr + s->node_off[g];
        const int64_t* h_ptr = sg.download(d_ptr, (size_t)(N + 1));
        GM_REQUIRE(h_ptr, GM_ENOMEM, "%s: pinned staging allocation failed", what);
        GM_HIP(hipMemcpyAsync(p->d, s->d_feat + s->node_off[g] * ld, (size_t)level * sizeof(float), hipMemcpyDeviceToDevice, st));      // level 0
        GM_HIP(hipStreamSynchronize(st));
        const int64_t e0 = h_ptr[0], nnz = h_ptr[N] - e0;
        GM_REQUIRE((nnz + GM_PR_THREADS - 1) / GM_PR_THREADS <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld edges pass the launch's 2^31 workgroups", what, (long long)nnz);
        const pr_graph G = {d_ptr, s->d_in_idx, s->weighted ? s->d_in_w : nullptr, N, e0, self};
        gm_col_hub_lists hl;
        if (self) {                                                            // the extended rows' pointers: one entry more per row
            std::vector<int64_t> ext((size_t)N + 1);
            for (int64_t v = 0; v <= N; ++v) ext[(size_t)v] = h_ptr[v] + v;
            GM_TRY(gm_col_hub_cut(what, ext.data(), N, C, 25, "prop_chunk", &hl));
        } else {
            GM_TRY(gm_col_hub_cut(what, h_ptr, N, C, 25, "prop_chunk", &hl));
        }
        gm_col_hubs<float> H;
        GM_TRY(gm_col_hubs_put(&H, hl, ld, sc, sg));
        float *norm = nullptr, *coef = nullptr;
        GM_TRY(sc.take(&norm, (size_t)N)); GM_TRY(sc.take(&coef, (size_t)nnz));
        gm_phase_timer tm(what);
        const dim3 block(GM_PR_THREADS);
        hipLaunchKernelGGL(k_prop_norm, dim3(pr_blocks(N)), block, 0, st, G, C, norm);
        if (H.n_hubs) {                                                        // (the degree sums borrow the first n_items floats of the partial rows)
            hipLaunchKernelGGL(k_prop_norm_parts, dim3(pr_blocks(H.n_items)), block, 0, st, G, C, (const int32_t*)H.it_row, (const int32_t*)H.it_seg, H.n_items, H.part);
            hipLaunchKernelGGL(k_prop_norm_hubs, dim3(pr_blocks(H.n_hubs)), block, 0, st, (const int32_t*)H.row, (const int32_t*)H.first, H.n_hubs, (const float*)H.part, norm);
        }
        if (nnz) hipLaunchKernelGGL(k_prop_coef, dim3(pr_blocks(nnz)), block, 0, st, G, nnz, (const float*)norm, coef);
        GM_HIP(hipGetLastError());
        if (tm.on) { GM_HIP(hipStreamSynchronize(st)); tm.lap("norm"); }
        if (ld >= 256) GM_TRY(pr_levels<4>(st, G, C, p, H, norm, coef, tm));                  // (ld is a multiple of 4: every row is 16-byte aligned)
        else if (ld >= 128) GM_TRY(pr_levels<2>(st, G, C, p, H, norm, coef, tm));
        else GM_TRY(pr_levels<1>(st, G, C, p, H, norm, coef, tm));
        GM_HIP(hipStreamSynchronize(st));                                      // complete on the device: afterwards any stream reads the levels without an event
    }
    own.p = nullptr;
    *out = p;
    return GM_OK;
}

extern "C" int32_t gm_prop_dims(const gm_prop_t* p, int64_t* n_nodes, int32_t* hops, int32_t* feat_dim, int32_t* flags, int64_t* bytes) {
    GM_REQUIRE(p, GM_EINVAL, "gm_prop_dims: prop is NULL");
    if (n_nodes) *n_nodes = p->N;
    if (hops) *hops = p->hops;
    if (feat_dim) *feat_dim = p->F;
    if (flags) *flags = p->flags;
    if (bytes) *bytes = p->bytes;
    return GM_OK;
}

// 16-byte accesses where the feature width and the caller's pointer allow them (the levels' rows always do: ld is a multiple of 4)
static inline bool pr_wide(const gm_prop* p, const float* d_out) { return p->F % 4 == 0 && ((uintptr_t)d_out & 15) == 0; }

extern "C" int32_t gm_prop_rows(const gm_prop_t* p, int32_t level, const int32_t* d_nodes, int64_t m, float* d_out, void* stream) {
    const char* what = "gm_prop_rows";
    GM_REQUIRE(p, GM_EINVAL, "%s: prop is NULL", what);
    GM_REQUIRE(level >= 0 && level <= p->hops, GM_EINVAL, "%s: level = %d of a propagation with hops = %d", what, level, p->hops);
    GM_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX, GM_EINVAL, "%s: m = %lld", what, (long long)m);
    if (m == 0) return GM_OK;
    GM_REQUIRE(d_nodes && d_out, GM_EINVAL, "%s: NULL argument", what);
    const float* lv = p->d + (int64_t)level * p->N * p->ld;
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = pr_wide(p, d_out);
    const int64_t threads = m * (wide ? p->F / 4 : p->F);
    GM_REQUIRE((threads + GM_PR_THREADS - 1) / GM_PR_THREADS <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld rows of %d columns pass the launch's 2^31 workgroups", what, (long long)m, p->F);
    if (wide) hipLaunchKernelGGL(k_prop_rows<4>, dim3(pr_blocks(threads)), dim3(GM_PR_THREADS), 0, st, lv, p->N, p->F, p->ld, d_nodes, m, d_out);
    else hipLaunchKernelGGL(k_prop_rows<1>, dim3(pr_blocks(threads)), dim3(GM_PR_THREADS), 0, st, lv, p->N, p->F, p->ld, d_nodes, m, d_out);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

extern "C" int32_t gm_prop_pair_features(const gm_prop_t* p, const int32_t* d_pairs, int64_t n, int32_t op, float* d_out, void* stream) {
    const char* what = "gm_prop_pair_features";
    GM_REQUIRE(p, GM_EINVAL, "%s: prop is NULL", what);
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    GM_REQUIRE(op == GM_PROP_HADAMARD || op == GM_PROP_ABS_DIFF, GM_EINVAL, "%s: op = %d; GM_PROP_HADAMARD = 0, GM_PROP_ABS_DIFF = 1", what, op);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out, GM_EINVAL, "%s: NULL argument", what);
    const int32_t L1 = p->hops + 1;
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = pr_wide(p, d_out);
    const int64_t threads = n * L1 * (wide ? p->F / 4 : p->F);
    GM_REQUIRE((threads + GM_PR_THREADS - 1) / GM_PR_THREADS <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld pairs of %d levels of %d columns pass the launch's 2^31 workgroups", what,
               (long long)n, L1, p->F);
    if (wide) hipLaunchKernelGGL(k_prop_pairs<4>, dim3(pr_blocks(threads)), dim3(GM_PR_THREADS), 0, st, (const float*)p->d, p->N, L1, p->F, p->ld, d_pairs, n, op, d_out);
    else hipLaunchKernelGGL(k_prop_pairs<1>, dim3(pr_blocks(threads)), dim3(GM_PR_THREADS), 0, st, (const float*)p->d, p->N, L1, p->F, p->ld, d_pairs, n, op, d_out);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
