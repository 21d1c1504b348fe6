// Held-out edges: a store derived on the device from a resident one with a set of node pairs removed (gm_store_without_edges), the deterministic edge
// split that produces such a set (gm_store_split_edges), and the read-backs that show what a store holds (gm_store_dims, gm_store_read_csr).  The
// DEFINITION is in include/gmeta_hip.h; tests/holdout_ref.py restates it and the GPU tests compare bit for bit.  This file is how it is computed:
//   an ENTRY ARRAY (the in-CSR, the by-source CSR, the neighbour index) is cut into chunks of GM_HO_CHUNK slots, one block each.
//     k_ho_flag     one thread per slot (GM_HO_PER slots a thread): the slot's row by a binary search of the row pointers, narrowed to the rows the
//                   chunk touches; the predicate (is the slot's canonical pair listed / which class does the hash give the link); one bit per slot
//                   (a wave's ballot is one 64-bit word, stored by one lane) and one kept-count per block.  A hub row is just more slots.
//     k_ho_scan     one block: exclusive prefix of the block counts in int64, the total behind the last block.
//     k_ho_compact  the kept slots written at block prefix + popcount of the chunk's words below the slot: the stored order survives by construction.
//     k_ho_ptr      new_ptr[row] = kept slots below old_ptr[row], from the same words.
//   Filtering keeps relative order, so the parent's by-source CSR filtered by the same predicate IS the by-source CSR of the result: both orientations
//   run the same kernels and nothing is sorted.  Integer work only: no atomics, nothing depends on arrival order.
// Everything runs on the caller's stream; scratch comes from the stream-ordered pool and goes back to it on that stream.
#include "gm_nbr.h"
#include "gm_devutil.h"      // lowbias32, sample_salt, gm_key_listed

#define GM_HO_THREADS 256
#define GM_HO_PER 4
#define GM_HO_CHUNK (GM_HO_THREADS * GM_HO_PER)      // slots per block
#define GM_HO_WORDS (GM_HO_CHUNK / 64)               // 64-bit keep words per block
#define GM_HO_SPLIT_TAG 0x53504C54                   // the `i` of sample_salt(seed, g, i, 0) for the split's hash

// slot s in [0, E) is entry e0 + s of the array; row r in [0, nrows) holds the entries [ptr[r], ptr[r + 1]); ptr[0] = e0, ptr[nrows] = e0 + E
struct ho_rows {
    const int64_t* ptr;
    int64_t nrows, e0, E;
};

// the last row in [lo, hi) that starts at or before entry e  (ptr[lo] <= e < ptr[hi])
__device__ __forceinline__ int64_t ho_row_of(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t e) {
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// the rows the block's chunk touches -> win[0] (row of its first slot), win[1] (one past the row of its last slot); behind a barrier
__device__ __forceinline__ void ho_row_window(const ho_rows& R, int64_t s0, int64_t* win) {
    if (threadIdx.x == 0 || threadIdx.x == GM_WAVE) {
        const int64_t last = s0 + GM_HO_CHUNK - 1 < R.E ? s0 + GM_HO_CHUNK - 1 : R.E - 1;
        const int64_t s = threadIdx.x == 0 ? s0 : last;
        win[threadIdx.x == 0 ? 0 : 1] = ho_row_of(R.ptr, 0, R.nrows, R.e0 + s) + (threadIdx.x == 0 ? 0 : 1);
    }
    __syncthreads();
}

// the graph of a global row / of a position in the concatenated key lists: the last g with off[g] <= x  (off[0] <= x < off[G])
__device__ __forceinline__ int32_t ho_graph_of(const int64_t* __restrict__ off, int32_t G, int64_t x) {
    int32_t lo = 0, hi = G;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Predicate of gm_store_without_edges over a CSR of the store (rows = global node ids, entries = the other endpoint, local): 1 = the slot stays.
// extra(): the check of the key lists themselves, spread over the launch's threads -- every key inside [0, N_g^2) and above its predecessor in the list.
struct ho_pred_keys {
    const int32_t* idx; const int64_t* node_off; int32_t G; const int64_t* keys; const int64_t* key_off; int64_t n_keys;      // n_keys = 0: no list check in this launch
    __device__ __forceinline__ int cls(int64_t e, int64_t row) const {
        const int32_t g = ho_graph_of(node_off, G, row);
        const int64_t no = node_off[g], N = node_off[g + 1] - no, a = row - no, b = idx[e];
        const int64_t key = (a < b ? a : b) * N + (a < b ? b : a);
        const int64_t k0 = key_off[g];
        return gm_key_listed(keys + k0, key_off[g + 1] - k0, key) ? 0 : 1;
    }
    __device__ __forceinline__ int extra(int64_t tid, int64_t nthreads) const {
        int bad = 0;
        for (int64_t i = tid; i < n_keys; i += nthreads) {
            const int32_t g = ho_graph_of(key_off, G, i);      // (empty lists share an offset: the LAST graph that starts at or before i is the one that holds it)
            const int64_t N = node_off[g + 1] - node_off[g], k = keys[i];
            if (k < 0 || k >= N * N || (i > key_off[g] && keys[i - 1] >= k)) ++bad;
        }
        return bad;
    }
};

// Predicate of gm_store_split_edges over the neighbour index of one graph (rows = local node ids): 0 = not a held-out link (v <= u, or class train),
// 1 = validation, 2 = test
struct ho_pred_split {
    const int32_t* idx; uint32_t s0; uint64_t t_test, t_val;
    __device__ __forceinline__ int cls(int64_t e, int64_t row) const {
        const int32_t u = (int32_t)row, v = idx[e];
        if (u >= v) return 0;
        const uint64_t h = lowbias32(lowbias32(s0 + (uint32_t)u) + (uint32_t)v);
        return h < t_test ? 2 : h < t_val ? 1 : 0;
    }
    __device__ __forceinline__ int extra(int64_t, int64_t) const { return 0; }
};

// bits[blocks * GM_HO_WORDS]: bit (s & 63) of word (s >> 6) = slot s stays;  blk[b] = kept slots of block b;  aux[b] = its slots of class 2 + its share of extra()
template <class Pred>
__global__ void __launch_bounds__(GM_HO_THREADS)
k_ho_flag(ho_rows R, Pred P, unsigned long long* __restrict__ bits, int32_t* __restrict__ blk, int32_t* __restrict__ aux) {
    __shared__ int64_t win[2];
    __shared__ int32_t cnt[2][GM_HO_THREADS / GM_WAVE];
    const int64_t s0 = (int64_t)blockIdx.x * GM_HO_CHUNK;
    const int lane = threadIdx.x & (GM_WAVE - 1), wave = threadIdx.x / GM_WAVE;
    if (s0 < R.E) ho_row_window(R, s0, win);      // (block-uniform; a launch over an empty array still has its one block for extra())
    int32_t kept = 0;
    int32_t two = P.extra((int64_t)blockIdx.x * GM_HO_THREADS + threadIdx.x, (int64_t)gridDim.x * GM_HO_THREADS);
#pragma unroll
    for (int it = 0; it < GM_HO_PER; ++it) {
        const int64_t s = s0 + it * GM_HO_THREADS + threadIdx.x;
        int c = 0;
        if (s < R.E) {
            const int64_t e = R.e0 + s;
            c = P.cls(e, ho_row_of(R.ptr, win[0], win[1], e));
        }
        const unsigned long long m = __ballot(c != 0);
        if (lane == 0) bits[(s0 >> 6) + it * (GM_HO_THREADS / GM_WAVE) + wave] = m;
        kept += __popcll(m);                          // (the same in every lane of the wave)
        two += c == 2 ? 1 : 0;
    }
    for (int d = GM_WAVE / 2; d >= 1; d >>= 1) two += __shfl_down(two, d, GM_WAVE);
    if (lane == 0) { cnt[0][wave] = kept; cnt[1][wave] = two; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t a = 0, b = 0;
        for (int w = 0; w < GM_HO_THREADS / GM_WAVE; ++w) { a += cnt[0][w]; b += cnt[1][w]; }
        blk[blockIdx.x] = a; aux[blockIdx.x] = b;
    }
}

// blk[0 .. nb) -> pref[0 .. nb] (exclusive prefix, the total at nb), tot = {sum of blk, sum of aux}: int64 throughout
__global__ void __launch_bounds__(1024) k_ho_scan(const int32_t* __restrict__ blk, const int32_t* __restrict__ aux, int32_t nb, int64_t* __restrict__ pref, int64_t* __restrict__ tot) {
    __shared__ int64_t buf[1024];
    __shared__ int64_t carry, carry_aux;
    if (threadIdx.x == 0) { carry = 0; carry_aux = 0; }
    __syncthreads();
    for (int32_t b0 = 0; b0 < nb; b0 += 1024) {
        const int32_t b = b0 + (int32_t)threadIdx.x;
        for (int pass = 0; pass < 2; ++pass) {
            const int64_t mine = b < nb ? (int64_t)(pass == 0 ? blk[b] : aux[b]) : 0;
            buf[threadIdx.x] = mine;
            __syncthreads();
            for (int d = 1; d < 1024; d <<= 1) {
                const int64_t add = (int)threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
                __syncthreads();
                buf[threadIdx.x] += add;
                __syncthreads();
            }
            if (pass == 0 && b < nb) pref[b] = carry + buf[threadIdx.x] - mine;
            __syncthreads();
            if (threadIdx.x == 1023) { if (pass == 0) carry += buf[1023]; else carry_aux += buf[1023]; }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) { pref[nb] = carry; tot[0] = carry; tot[1] = carry_aux; }
}

// kept slots below slot s, 0 <= s <= E
__device__ __forceinline__ int64_t ho_kept_below(const unsigned long long* __restrict__ bits, const int64_t* __restrict__ pref, int32_t nb, int64_t E, int64_t s) {
    if (s >= E) return pref[nb];
    const int64_t b = s / GM_HO_CHUNK, w = s >> 6;
    int64_t r = pref[b];
    for (int64_t j = b * GM_HO_WORDS; j < w; ++j) r += __popcll(bits[j]);
    return r + __popcll(bits[w] & ((1ull << (s & 63)) - 1ull));
}

// what a kept slot becomes.  A CSR of the derived store: the entry and its weight move to their new position.
struct ho_emit_csr {
    static constexpr bool needs_row = false;
    const int32_t* idx; const float* w; int32_t* new_idx; float* new_w;
    __device__ __forceinline__ void operator()(int64_t pos, int64_t e, int64_t) const {
        new_idx[pos] = idx[e];
        if (w) new_w[pos] = w[e];
    }
};
// The split: the pair (row, entry) and its class.  Rows ascend, entries ascend inside a row and u < v: the pairs come out in ascending u * N + v.
struct ho_emit_split {
    static constexpr bool needs_row = true;
    ho_pred_split P; int32_t* pairs; uint8_t* cls;
    __device__ __forceinline__ void operator()(int64_t pos, int64_t e, int64_t row) const {
        pairs[2 * pos] = (int32_t)row; pairs[2 * pos + 1] = P.idx[e];
        if (cls) cls[pos] = (uint8_t)P.cls(e, row);
    }
};

template <class Emit>
__global__ void __launch_bounds__(GM_HO_THREADS)
k_ho_compact(ho_rows R, Emit emit, const unsigned long long* __restrict__ bits, const int64_t* __restrict__ pref) {
    __shared__ int64_t win[2];
    __shared__ unsigned long long wd[GM_HO_WORDS];
    __shared__ int32_t below[GM_HO_WORDS];
    const int64_t s0 = (int64_t)blockIdx.x * GM_HO_CHUNK;
    if (threadIdx.x < GM_HO_WORDS) wd[threadIdx.x] = bits[(s0 >> 6) + threadIdx.x];
    if (Emit::needs_row) ho_row_window(R, s0, win);      // (every block of this launch holds a slot: the grid is cut from E >= 1)
    else __syncthreads();
    if (threadIdx.x == 0) { int32_t t = 0; for (int j = 0; j < GM_HO_WORDS; ++j) { below[j] = t; t += __popcll(wd[j]); } }
    __syncthreads();
    const int64_t base = pref[blockIdx.x];
#pragma unroll
    for (int it = 0; it < GM_HO_PER; ++it) {
        const int32_t in_blk = it * GM_HO_THREADS + (int32_t)threadIdx.x;
        const unsigned long long m = wd[in_blk >> 6];
        if (!((m >> (in_blk & 63)) & 1ull)) continue;      // (slots at or beyond E never carry a bit)
        const int64_t e = R.e0 + s0 + in_blk;
        const int64_t pos = base + below[in_blk >> 6] + __popcll(m & ((1ull << (in_blk & 63)) - 1ull));
        emit(pos, e, Emit::needs_row ? ho_row_of(R.ptr, win[0], win[1], e) : 0);
    }
}

__global__ void __launch_bounds__(GM_HO_THREADS)
k_ho_ptr(ho_rows R, const unsigned long long* __restrict__ bits, const int64_t* __restrict__ pref, int32_t nb, int64_t* __restrict__ new_ptr) {
    const int64_t r = (int64_t)blockIdx.x * GM_HO_THREADS + threadIdx.x;
    if (r > R.nrows) return;
    new_ptr[r] = ho_kept_below(bits, pref, nb, R.E, R.ptr[r] - R.e0);
}

// *diff = 1 where the two CSRs differ in any word (row pointers, entries, weights): the store's `symmetric` flag is its negation.  Every writer stores
// the same value.
__global__ void __launch_bounds__(GM_HO_THREADS)
k_ho_differ(const int64_t* __restrict__ pa, const int64_t* __restrict__ pb, int64_t np, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
            const float* __restrict__ wa, const float* __restrict__ wb, int64_t ne, int32_t* __restrict__ diff) {
    const int64_t i0 = (int64_t)blockIdx.x * GM_HO_THREADS + threadIdx.x, step = (int64_t)gridDim.x * GM_HO_THREADS;
    bool d = false;
    for (int64_t i = i0; i < np; i += step) d |= pa[i] != pb[i];
    for (int64_t i = i0; i < ne; i += step) d |= ia[i] != ib[i];
    if (wa)
        for (int64_t i = i0; i < ne; i += step) d |= wa[i] != wb[i];
    if (d) *diff = 1;
}

// edge_off[g] = in_ptr[node_off[g]]
__global__ void k_ho_edge_off(const int64_t* __restrict__ in_ptr, const int64_t* __restrict__ node_off, int32_t n, int64_t* __restrict__ out) {
    const int32_t g = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g < n) out[g] = in_ptr[node_off[g]];
}

// ---- host

static inline int32_t ho_blocks(int64_t E) { return (int32_t)std::max<int64_t>(1, (E + GM_HO_CHUNK - 1) / GM_HO_CHUNK); }

// the keep words, the block prefix and the totals of one flag + scan over an entry array
struct ho_marks {
    unsigned long long* bits = nullptr; int32_t* blk = nullptr; int32_t* aux = nullptr; int64_t* pref = nullptr; int64_t* tot = nullptr; int32_t nb = 0;
};

// laps of GM_TIMING=1: the stream is drained behind each phase only while the timer prints
static inline void ho_lap(gm_phase_timer& tm, hipStream_t st, const char* phase) {
    if (!tm.on) return;
    (void)hipStreamSynchronize(st);
    tm.lap(phase);
}

template <class Pred>
static int ho_mark(const char* what, const ho_rows& R, const Pred& P, gm_scratch& sc, hipStream_t st, ho_marks* m, gm_phase_timer& tm) {
    GM_REQUIRE(R.E <= (int64_t)INT32_MAX * (GM_HO_CHUNK / 2), GM_ERANGE, "%s: %lld entries: more blocks than one launch holds", what, (long long)R.E);
    m->nb = ho_blocks(R.E);
    GM_TRY(sc.take(&m->bits, (size_t)m->nb * GM_HO_WORDS));
    GM_TRY(sc.take(&m->blk, (size_t)m->nb));
    GM_TRY(sc.take(&m->aux, (size_t)m->nb));
    GM_TRY(sc.take(&m->pref, (size_t)m->nb + 1));
    GM_TRY(sc.take(&m->tot, 2));
    hipLaunchKernelGGL(k_ho_flag<Pred>, dim3((unsigned)m->nb), dim3(GM_HO_THREADS), 0, st, R, P, m->bits, m->blk, m->aux);
    ho_lap(tm, st, "flag");
    hipLaunchKernelGGL(k_ho_scan, dim3(1), dim3(1024), 0, st, (const int32_t*)m->blk, (const int32_t*)m->aux, m->nb, m->pref, m->tot);
    GM_HIP(hipGetLastError());
    ho_lap(tm, st, "scan");
    return GM_OK;
}

template <class Emit>
static int ho_compact(const ho_rows& R, const Emit& emit, const ho_marks& m, hipStream_t st) {
    if (R.E <= 0) return GM_OK;
    hipLaunchKernelGGL(k_ho_compact<Emit>, dim3((unsigned)m.nb), dim3(GM_HO_THREADS), 0, st, R, emit, (const unsigned long long*)m.bits, (const int64_t*)m.pref);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

static int without_edges(const gm_store* s, const int64_t* d_keys, const int64_t* h_key_off, gm_store* o, hipStream_t st) {
    const char* what = "gm_store_without_edges";
    gm_phase_timer tm("without_edges");
    const int32_t G = s->n_graphs;
    const int64_t T = s->total_nodes, E = s->total_edges, K = h_key_off[G];
    gm_scratch sc(st);
    gm_stager sg(st);
    int64_t* d_key_off = nullptr;
    GM_TRY(sc.take(&d_key_off, (size_t)G + 1));
    GM_TRY(sg.upload((void*)d_key_off, (const void*)h_key_off, ((size_t)G + 1) * sizeof(int64_t)));

    // flag + scan, both orientations; the in-CSR's launch also checks the key lists
    const ho_rows Rin = {s->d_in_ptr, T, 0, E}, Rout = {s->d_out_ptr, T, 0, E};
    ho_marks m_in, m_out;
    GM_TRY(ho_mark(what, Rin, ho_pred_keys{s->d_in_idx, s->d_node_off, G, d_keys, d_key_off, K}, sc, st, &m_in, tm));
    GM_TRY(ho_mark(what, Rout, ho_pred_keys{s->d_out_idx, s->d_node_off, G, d_keys, d_key_off, 0}, sc, st, &m_out, tm));
    int64_t* h_in = sg.download((const int64_t*)m_in.tot, 2);
    int64_t* h_out = sg.download((const int64_t*)m_out.tot, 2);
    GM_REQUIRE(h_in && h_out, GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(st));
    tm.lap("counts read back");
    GM_REQUIRE(h_in[1] == 0, GM_EINVAL, "%s: %lld key(s) outside [0, N_g^2) or not strictly ascending inside their graph's list", what, (long long)h_in[1]);
    GM_REQUIRE(h_in[0] == h_out[0], GM_EHIP, "%s: the two orientations kept %lld and %lld edges", what, (long long)h_in[0], (long long)h_out[0]);
    const int64_t E2 = h_in[0];

    // the derived store: the host side, then the arrays
    o->n_graphs = G; o->feat_dim = s->feat_dim; o->feat_ld = s->feat_ld;
    o->total_nodes = T; o->total_edges = E2; o->max_nodes = s->max_nodes; o->weighted = s->weighted;
    o->node_off = s->node_off; o->h_feat_amax = s->h_feat_amax; o->h_feat_mean = s->h_feat_mean;
    GM_TRY(gm_alloc(&o->d_node_off, (size_t)G + 1, st));
    GM_TRY(gm_alloc(&o->d_in_ptr, (size_t)T + 1, st));
    GM_TRY(gm_alloc(&o->d_out_ptr, (size_t)T + 1, st));
    GM_TRY(gm_alloc(&o->d_in_idx, (size_t)E2, st));
    GM_TRY(gm_alloc(&o->d_out_idx, (size_t)E2, st));
    if (s->weighted) { GM_TRY(gm_alloc(&o->d_in_w, (size_t)E2, st)); GM_TRY(gm_alloc(&o->d_out_w, (size_t)E2, st)); }
    if (E2 == 0) {      // gm_store_create uploads one zero entry (and one unit weight) for a store without edges
        GM_HIP(hipMemsetAsync(o->d_in_idx, 0, sizeof(int32_t), st)); GM_HIP(hipMemsetAsync(o->d_out_idx, 0, sizeof(int32_t), st));
        if (s->weighted) { GM_HIP(hipMemsetD32Async((hipDeviceptr_t)o->d_in_w, 0x3F800000, 1, st)); GM_HIP(hipMemsetD32Async((hipDeviceptr_t)o->d_out_w, 0x3F800000, 1, st)); }
    }
    GM_HIP(hipMemcpyAsync(o->d_node_off, s->d_node_off, ((size_t)G + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    GM_TRY(ho_compact(Rin, ho_emit_csr{s->d_in_idx, s->d_in_w, o->d_in_idx, o->d_in_w}, m_in, st));
    GM_TRY(ho_compact(Rout, ho_emit_csr{s->d_out_idx, s->d_out_w, o->d_out_idx, o->d_out_w}, m_out, st));
    const dim3 pgrid((unsigned)((T + 1 + GM_HO_THREADS - 1) / GM_HO_THREADS));
    hipLaunchKernelGGL(k_ho_ptr, pgrid, dim3(GM_HO_THREADS), 0, st, Rin, (const unsigned long long*)m_in.bits, (const int64_t*)m_in.pref, m_in.nb, o->d_in_ptr);
    hipLaunchKernelGGL(k_ho_ptr, pgrid, dim3(GM_HO_THREADS), 0, st, Rout, (const unsigned long long*)m_out.bits, (const int64_t*)m_out.pref, m_out.nb, o->d_out_ptr);
    GM_HIP(hipGetLastError());
    ho_lap(tm, st, "compact");

    int32_t* d_diff = nullptr; int64_t* d_edge_off = nullptr;
    GM_TRY(sc.take(&d_diff, 1));
    GM_TRY(sc.take(&d_edge_off, (size_t)G + 1));
    GM_HIP(hipMemsetAsync(d_diff, 0, sizeof(int32_t), st));
    if (E2 > 0) {
        const int64_t most = std::max<int64_t>(T + 1, E2);
        const unsigned grid = (unsigned)std::min<int64_t>((most + GM_HO_THREADS - 1) / GM_HO_THREADS, 4096);
        hipLaunchKernelGGL(k_ho_differ, dim3(grid), dim3(GM_HO_THREADS), 0, st, (const int64_t*)o->d_in_ptr, (const int64_t*)o->d_out_ptr, T + 1,
                           (const int32_t*)o->d_in_idx, (const int32_t*)o->d_out_idx, (const float*)o->d_in_w, (const float*)o->d_out_w, E2, d_diff);
    }
    hipLaunchKernelGGL(k_ho_edge_off, dim3((unsigned)((G + 1 + 63) / 64)), dim3(64), 0, st, (const int64_t*)o->d_in_ptr, (const int64_t*)o->d_node_off, G + 1, d_edge_off);
    GM_HIP(hipGetLastError());
    ho_lap(tm, st, "symmetric check");

    // the features: the same table, the same bound, device to device
    GM_TRY(gm_dev_alloc((void**)&o->d_feat, (size_t)T * s->feat_ld * sizeof(float), st));
    GM_TRY(gm_alloc(&o->d_feat_amax, 1, st));
    GM_HIP(hipMemcpyAsync(o->d_feat, s->d_feat, (size_t)T * s->feat_ld * sizeof(float), hipMemcpyDeviceToDevice, st));
    GM_HIP(hipMemcpyAsync(o->d_feat_amax, s->d_feat_amax, sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    ho_lap(tm, st, "feature copy");

    int32_t* h_diff = sg.download((const int32_t*)d_diff, 1);
    int64_t* h_edge_off = sg.download((const int64_t*)d_edge_off, (size_t)G + 1);
    GM_REQUIRE(h_diff && h_edge_off, GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(st));
    o->edge_off.assign(h_edge_off, h_edge_off + G + 1);
    o->symmetric = E2 > 0 && *h_diff == 0 && getenv("GM_EXTRACT_NO_SYM") == nullptr;
    tm.lap("read back");
    return GM_OK;
}

extern "C" int32_t gm_store_without_edges(const gm_store_t* s, const int64_t* d_keys, const int64_t* h_key_off, gm_store_t** out, void* stream) {
    const char* what = "gm_store_without_edges";
    GM_REQUIRE(out, GM_EINVAL, "%s: out is NULL", what);
    *out = nullptr;
    GM_REQUIRE(s && h_key_off, GM_EINVAL, "%s: NULL argument", what);
    GM_REQUIRE(h_key_off[0] == 0, GM_EINVAL, "%s: h_key_off[0] = %lld, not 0", what, (long long)h_key_off[0]);
    for (int32_t g = 0; g < s->n_graphs; ++g)
        GM_REQUIRE(h_key_off[g + 1] >= h_key_off[g], GM_EINVAL, "%s: h_key_off is not monotone at graph %d", what, g);
    GM_REQUIRE(d_keys || h_key_off[s->n_graphs] == 0, GM_EINVAL, "%s: d_keys is NULL with %lld key(s) listed", what, (long long)h_key_off[s->n_graphs]);
    gm_store* o = new gm_store();
    const int rc = without_edges(s, d_keys, h_key_off, o, (hipStream_t)stream);
    if (rc != GM_OK) { gm_store_destroy(o); return rc; }
    *out = o;
    return GM_OK;
}

extern "C" int32_t gm_store_split_edges(const gm_store_t* s, int32_t g, uint64_t seed, uint64_t t_test, uint64_t t_val, int32_t* d_out_pairs, uint8_t* d_out_class,
                                        int64_t capacity, int64_t* h_counts, void* stream) {
    const char* what = "gm_store_split_edges";
    GM_REQUIRE(h_counts, GM_EINVAL, "%s: h_counts is NULL", what);
    h_counts[0] = h_counts[1] = h_counts[2] = 0;
    GM_TRY(gm_store_call_check(what, s, g));
    GM_REQUIRE(t_test <= t_val && t_val <= (1ull << 32), GM_EINVAL, "%s: thresholds %llu, %llu: 0 <= t_test <= t_val <= 2^32", what, (unsigned long long)t_test,
               (unsigned long long)t_val);
    GM_REQUIRE(capacity >= 0, GM_EINVAL, "%s: capacity = %lld", what, (long long)capacity);
    GM_TRY(gm_nbr_index(s));
    hipStream_t st = (hipStream_t)stream;
    const gm_nbr_graph NG = gm_nbr_graph_of(s, g);
    const ho_rows R = {NG.ptr, NG.N, s->nbr_off[g], s->nbr_off[g + 1] - s->nbr_off[g]};
    const ho_pred_split P = {NG.idx, sample_salt(seed, g, GM_HO_SPLIT_TAG, 0), t_test, t_val};
    gm_phase_timer tm("split_edges");
    gm_scratch sc(st);
    gm_stager sg(st);
    ho_marks m;
    GM_TRY(ho_mark(what, R, P, sc, st, &m, tm));
    int64_t* h_tot = sg.download((const int64_t*)m.tot, 2);
    GM_REQUIRE(h_tot, GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(st));
    const int64_t held = h_tot[0], test = h_tot[1];
    h_counts[0] = R.E / 2;      // the rows are symmetric and hold no node twice: every link sits in two of them
    h_counts[1] = held - test; h_counts[2] = test;
    if (!d_out_pairs) return GM_OK;
    GM_REQUIRE(capacity >= held, GM_ERANGE, "%s: capacity %lld for %lld held-out pair(s)", what, (long long)capacity, (long long)held);
    if (held == 0) return GM_OK;
    GM_TRY(ho_compact(R, ho_emit_split{P, d_out_pairs, d_out_class}, m, st));
    GM_HIP(hipStreamSynchronize(st));      // the scratch goes back behind the kernels; the pairs are complete when the call returns
    tm.lap("compact");
    return GM_OK;
}

extern "C" int32_t gm_store_dims(const gm_store_t* s, int32_t g, int64_t* n_nodes, int64_t* n_edges, int32_t* symmetric) {
    GM_TRY(gm_store_call_check("gm_store_dims", s, g));
    if (n_nodes) *n_nodes = s->node_off[g + 1] - s->node_off[g];
    if (n_edges) *n_edges = s->edge_off[g + 1] - s->edge_off[g];
    if (symmetric) *symmetric = s->symmetric ? 1 : 0;
    return GM_OK;
}

extern "C" int32_t gm_store_read_csr(const gm_store_t* s, int32_t g, int32_t orientation, int64_t* h_ptr, int32_t* h_idx, float* h_w) {
    const char* what = "gm_store_read_csr";
    GM_TRY(gm_store_call_check(what, s, g));
    GM_REQUIRE(orientation == 0 || orientation == 1, GM_EINVAL, "%s: orientation %d (0 = by destination, 1 = by source)", what, orientation);
    GM_REQUIRE(h_ptr && h_idx, GM_EINVAL, "%s: NULL argument", what);
    GM_REQUIRE(!h_w || s->weighted, GM_EINVAL, "%s: h_w given for a store without edge weights", what);
    const int64_t no = s->node_off[g], N = s->node_off[g + 1] - no, eo = s->edge_off[g], ne = s->edge_off[g + 1] - eo;
    GM_HIP(hipMemcpy(h_ptr, (orientation ? s->d_out_ptr : s->d_in_ptr) + no, (size_t)(N + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t v = 0; v <= N; ++v) h_ptr[v] -= eo;
    if (ne) {
        GM_HIP(hipMemcpy(h_idx, (orientation ? s->d_out_idx : s->d_in_idx) + eo, (size_t)ne * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (h_w) GM_HIP(hipMemcpy(h_w, (orientation ? s->d_out_w : s->d_in_w) + eo, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost));
    }
    return GM_OK;
}
