// Negative pairs for link prediction, drawn on the device from a store's parent graph (gm_store_negative_pairs), and the adjacency test they rest on
// (gm_store_has_edges).  The DEFINITION -- random words, candidate k, validity, order, budget -- is in include/gmeta_hip.h; tests/negative_ref.py restates
// it one candidate at a time and the GPU tests compare bit for bit.  This file is how it is computed:
//   the candidate stream k = 0, 1, 2, ... is cut into rounds of R candidates (R: gm_set_tuning("neg_round"), default by n).  Per round
//     k_neg_mark   one thread per candidate: the pair, its validity (two binary searches in the out-CSR, one in the exclusion keys); a valid pair claims a
//                  slot of an open-addressing table of int64 keys (64-bit compare-and-swap) and leaves min(k) there (integer atomic minimum);
//     k_neg_keep   candidate k survives iff it is valid and the table holds k for its key -- its first occurrence over ALL rounds so far, since the table
//                  lives through the call; per-block survivor counts;
//     k_neg_scan   one block: exclusive prefix of the block counts, behind the pairs found in the earlier rounds;
//     k_neg_emit   survivors written in k order at their prefix position, while that is below n.
//   Both atomics are order-independent in what they leave (which slot a key sits in may differ from run to run; the k stored for it cannot), so the
//   output is a function of the definition alone: not of R, not of the schedule.  The host reads one counter per round and stops at n or at the budget.
// Everything runs on the caller's stream; the table and the scratch come from the stream-ordered pool and go back to it on that stream.
#include "gm_internal.h"
#include "gm_devutil.h"      // lowbias32, sample_salt: extract.hip's hash and salt (oracle.lowbias32 / oracle.sample_salt); gm_key_listed: the search of the exclusion keys

#define GM_NEG_SALT_TAG 0x6E454721      // the `i` of sample_salt(seed, g, i, mode) for this stream of random words
#define GM_NEG_THREADS 256
#define GM_NEG_MAX_ROUND (1 << 22)      // candidates per round at most (8 bytes of scratch each)
#define GM_NEG_EMPTY 0xFFFFFFFFFFFFFFFFull

// one parent graph of a store: out-CSR rows by LOCAL node id, edge offsets global (into out_idx), destinations local
struct neg_graph {
    const int64_t* out_ptr;      // gm_store::d_out_ptr + node_off[g]   [N + 1]
    const int32_t* out_idx;      // gm_store::d_out_idx
    int64_t N;
};

__device__ __forceinline__ int64_t pick(uint32_t r, int64_t n) { return (int64_t)(((uint64_t)r * (uint64_t)n) >> 32); }

// INVARIANT the searches rest on (store.hip): the out-CSR is grouped by source and, inside a row, keeps the order in which the in-CSR
// lists the edges -- rows of ascending destination, walked by a stable counting sort -- so the destinations of an out-row ASCEND, parallel copies side
// by side.  (The in-CSR's rows keep the caller's edge order and are not sorted: only the out-rows can be searched.)  tests/test_negative_restatement.py
// checks the order on the host arrays.  A hub row costs log2(degree) loads here, so no wave-cooperative scan is needed.
__device__ __forceinline__ bool row_has(const neg_graph& G, int32_t u, int32_t v) {
    int64_t lo = G.out_ptr[u], hi = G.out_ptr[u + 1];
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int32_t x = G.out_idx[mid];
        if (x == v) return true;
        if (x < v) lo = mid + 1; else hi = mid;
    }
    return false;
}
// an edge u -> v or v -> u, at any multiplicity
__device__ __forceinline__ bool adjacent(const neg_graph& G, int32_t u, int32_t v) { return row_has(G, u, v) || (u != v && row_has(G, v, u)); }

// candidate k in canonical form; false where the definition calls it invalid before any look at the pair (a dead end of the walk, u == v)
__device__ __forceinline__ bool candidate(const neg_graph& G, uint32_t salt, int mode, uint32_t k, int32_t& u, int32_t& v) {
    const uint32_t w0 = salt + 4u * k;
    const int32_t a = (int32_t)pick(lowbias32(w0), G.N);
    int32_t b;
    if (mode == GM_NEG_UNIFORM) {
        b = (int32_t)pick(lowbias32(w0 + 1u), G.N);
    } else {
        const int64_t a0 = G.out_ptr[a], da = G.out_ptr[a + 1] - a0;
        if (da == 0) return false;
        const int32_t w = G.out_idx[a0 + pick(lowbias32(w0 + 1u), da)];
        const int64_t b0 = G.out_ptr[w], dw = G.out_ptr[w + 1] - b0;
        if (dw == 0) return false;
        b = G.out_idx[b0 + pick(lowbias32(w0 + 2u), dw)];
    }
    u = a < b ? a : b; v = a < b ? b : a;
    return u != v;
}

__device__ __forceinline__ uint32_t key_hash(int64_t key) { return lowbias32((uint32_t)key ^ lowbias32((uint32_t)((uint64_t)key >> 32) + 0x9E3779B9u)); }

__global__ void __launch_bounds__(GM_NEG_THREADS)
k_neg_mark(neg_graph G, uint32_t salt, int mode, const int64_t* excl, int64_t n_excl, uint32_t k0, int32_t cnt, int2* cand, unsigned long long* tab_key, int32_t* tab_k,
           uint32_t mask) {
    const int32_t i = (int32_t)(blockIdx.x * GM_NEG_THREADS + threadIdx.x);
    if (i >= cnt) return;
    const uint32_t k = k0 + (uint32_t)i;
    int32_t u = -1, v = -1;
    bool ok = candidate(G, salt, mode, k, u, v);
    const int64_t key = (int64_t)u * G.N + v;
    ok = ok && !adjacent(G, u, v) && !gm_key_listed(excl, n_excl, key);
    cand[i] = ok ? make_int2(u, v) : make_int2(-1, -1);
    if (!ok) return;
    // the table holds more than twice the keys a call can insert (the host sizes it): a free slot always ends the probe; the bound is a second fence
    uint32_t h = key_hash(key) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1u) & mask) {
        const unsigned long long was = atomicCAS(&tab_key[h], GM_NEG_EMPTY, (unsigned long long)key);
        if (was == GM_NEG_EMPTY || was == (unsigned long long)key) { atomicMin(&tab_k[h], (int32_t)k); return; }
    }
}

// survivors of each of the block's waves -> lds[0 .. 4) (behind a barrier); returns the survivors in the lanes below this one
__device__ __forceinline__ int block_count(bool keep, int32_t* lds) {
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & (GM_WAVE - 1)) == 0) lds[threadIdx.x / GM_WAVE] = __popcll(m);
    __syncthreads();
    return __popcll(m & ((1ull << (threadIdx.x & (GM_WAVE - 1))) - 1ull));
}

__global__ void __launch_bounds__(GM_NEG_THREADS)
k_neg_keep(int64_t N, uint32_t k0, int32_t cnt, int2* cand, const unsigned long long* tab_key, const int32_t* tab_k, uint32_t mask, int32_t* blk) {
    __shared__ int32_t lds[GM_NEG_THREADS / GM_WAVE];
    const int32_t i = (int32_t)(blockIdx.x * GM_NEG_THREADS + threadIdx.x);
    bool keep = false;
    if (i < cnt) {
        const int2 c = cand[i];
        if (c.x >= 0) {
            const unsigned long long key = (unsigned long long)((int64_t)c.x * N + c.y);
            uint32_t h = key_hash((int64_t)key) & mask;
            for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1u) & mask) {
                const unsigned long long at = tab_key[h];
                if (at == key) { keep = tab_k[h] == (int32_t)(k0 + (uint32_t)i); break; }
                if (at == GM_NEG_EMPTY) break;                                  // (never: k_neg_mark inserted it)
            }
            if (!keep) cand[i] = make_int2(-1, -1);                             // a later copy of a pair that counts where its smallest k is
        }
    }
    block_count(keep, lds);
    if (threadIdx.x == 0) { int32_t t = 0; for (int w = 0; w < GM_NEG_THREADS / GM_WAVE; ++w) t += lds[w]; blk[blockIdx.x] = t; }
}

// blk[0 .. nb) -> exclusive prefix, in place; state = {pairs found before this round, pairs found after it (capped at n)}
__global__ void __launch_bounds__(1024) k_neg_scan(int32_t* blk, int32_t nb, int32_t* state, int32_t n) {
    __shared__ int32_t buf[1024];
    __shared__ int32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int32_t b0 = 0; b0 < nb; b0 += 1024) {
        const int32_t b = b0 + (int32_t)threadIdx.x;
        const int32_t mine = b < nb ? blk[b] : 0;
        buf[threadIdx.x] = mine;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int32_t add = (int)threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        const int32_t base = carry;
        if (b < nb) blk[b] = base + buf[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 1023) carry = base + buf[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int32_t before = state[1];
        const int64_t after = (int64_t)before + carry;
        state[0] = before;
        state[1] = after < n ? (int32_t)after : n;
    }
}

__global__ void __launch_bounds__(GM_NEG_THREADS)
k_neg_emit(int32_t cnt, const int2* cand, const int32_t* blk, const int32_t* state, int32_t n, int32_t* out) {
    __shared__ int32_t lds[GM_NEG_THREADS / GM_WAVE];
    const int32_t i = (int32_t)(blockIdx.x * GM_NEG_THREADS + threadIdx.x);
    const int2 c = i < cnt ? cand[i] : make_int2(-1, -1);
    const bool keep = c.x >= 0;
    int64_t pos = (int64_t)state[0] + blk[blockIdx.x] + block_count(keep, lds);
    for (int w = 0; w < (int)(threadIdx.x / GM_WAVE); ++w) pos += lds[w];
    if (keep && pos < n) { out[2 * pos] = c.x; out[2 * pos + 1] = c.y; }       // the selection stops at n
}

__global__ void __launch_bounds__(GM_NEG_THREADS) k_has_edges(neg_graph G, const int32_t* pairs, int64_t n, uint8_t* out) {
    const int64_t i = (int64_t)blockIdx.x * GM_NEG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
    const bool in = a >= 0 && a < G.N && b >= 0 && b < G.N;                    // a node outside the graph has no edges
    out[i] = in && adjacent(G, a, b) ? 1 : 0;
}

static neg_graph neg_graph_of(const gm_store* s, int32_t g) { return {s->d_out_ptr + s->node_off[g], s->d_out_idx, s->node_off[g + 1] - s->node_off[g]}; }

extern "C" int32_t gm_store_negative_pairs(const gm_store_t* s, int32_t g, int64_t n, uint64_t seed, int32_t mode, const int64_t* d_exclude_keys, int64_t n_exclude,
                                           int32_t* d_out_pairs, int64_t* h_found, void* stream) {
    const char* what = "gm_store_negative_pairs";
    GM_REQUIRE(h_found, GM_EINVAL, "%s: h_found is NULL", what);
    *h_found = 0;
    GM_TRY(gm_store_call_check(what, s, g));
    const neg_graph G = neg_graph_of(s, g);
    GM_REQUIRE(G.N >= 2, GM_EINVAL, "%s: graph %d has %lld node(s); a pair needs two", what, g, (long long)G.N);
    GM_REQUIRE(mode == GM_NEG_UNIFORM || mode == GM_NEG_TWO_HOP, GM_EINVAL, "%s: unknown mode %d (GM_NEG_UNIFORM = 0, GM_NEG_TWO_HOP = 1)", what, mode);
    GM_REQUIRE(n >= 0, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    const int64_t n_max = ((int64_t)INT32_MAX - 4096) / 64;
    GM_REQUIRE(n <= n_max, GM_EINVAL, "%s: n = %lld: the draw budget 64 n + 4096 must fit the kernels' int32 counters (n <= %lld)", what, (long long)n, (long long)n_max);
    GM_REQUIRE(n_exclude >= 0 && (n_exclude == 0 || d_exclude_keys), GM_EINVAL, "%s: bad exclusion list", what);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_out_pairs, GM_EINVAL, "%s: d_out_pairs is NULL", what);
    hipStream_t st = (hipStream_t)stream;
    const int64_t budget = 64 * n + 4096;
    // Round size.  A sparse graph accepts nearly every candidate, so n + n / 4 + 4096 ends most calls in one round and the rest in two; the result does not
    // depend on it.  The table must hold every key a call inserts: fewer than n before the last round (or the call had stopped) plus one round's.
    int64_t R = gm_knob().neg_round > 0 ? gm_knob().neg_round : n + n / 4 + 4096;
    R = std::min<int64_t>(std::min<int64_t>(R, GM_NEG_MAX_ROUND), budget);
    uint64_t cap = 1024;
    while (cap < 2 * (uint64_t)(n + R)) cap <<= 1;
    const int32_t nb = (int32_t)((R + GM_NEG_THREADS - 1) / GM_NEG_THREADS);

    gm_scratch sc(st);
    unsigned long long* tab_key = nullptr; int32_t* tab_k = nullptr; int2* cand = nullptr; int32_t* blk = nullptr; int32_t* state = nullptr;
    GM_TRY(sc.take(&tab_key, cap));
    GM_TRY(sc.take(&tab_k, cap));
    GM_TRY(sc.take(&cand, (size_t)R));
    GM_TRY(sc.take(&blk, (size_t)nb));
    GM_TRY(sc.take(&state, 2));
    GM_HIP(hipMemsetAsync(tab_key, 0xFF, cap * sizeof(unsigned long long), st));
    GM_HIP(hipMemsetD32Async((hipDeviceptr_t)tab_k, INT32_MAX, cap, st));
    GM_HIP(hipMemsetAsync(state, 0, 2 * sizeof(int32_t), st));
    gm_stager sg(st);
    int32_t* h_state = (int32_t*)sg.take(sizeof(int32_t));
    GM_REQUIRE(h_state, GM_ENOMEM, "%s: pinned staging allocation failed", what);

    const uint32_t salt = sample_salt(seed, g, GM_NEG_SALT_TAG, mode), mask = (uint32_t)(cap - 1);
    int64_t found = 0;
    for (int64_t k0 = 0; k0 < budget && found < n; k0 += R) {
        const int32_t cnt = (int32_t)std::min<int64_t>(R, budget - k0);
        const dim3 grid((unsigned)((cnt + GM_NEG_THREADS - 1) / GM_NEG_THREADS)), block(GM_NEG_THREADS);
        hipLaunchKernelGGL(k_neg_mark, grid, block, 0, st, G, salt, (int)mode, d_exclude_keys, n_exclude, (uint32_t)k0, cnt, cand, tab_key, tab_k, mask);
        hipLaunchKernelGGL(k_neg_keep, grid, block, 0, st, G.N, (uint32_t)k0, cnt, cand, (const unsigned long long*)tab_key, (const int32_t*)tab_k, mask, blk);
        hipLaunchKernelGGL(k_neg_scan, dim3(1), dim3(1024), 0, st, blk, (int32_t)grid.x, state, (int32_t)n);
        hipLaunchKernelGGL(k_neg_emit, grid, block, 0, st, cnt, (const int2*)cand, (const int32_t*)blk, (const int32_t*)state, (int32_t)n, d_out_pairs);
        GM_HIP(hipGetLastError());
        GM_HIP(hipMemcpyAsync(h_state, state + 1, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        GM_HIP(hipStreamSynchronize(st));
        found = *h_state;
    }
    *h_found = found;
    return GM_OK;
}

extern "C" int32_t gm_store_has_edges(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, uint8_t* d_out, void* stream) {
    const char* what = "gm_store_has_edges";
    GM_TRY(gm_store_call_check(what, s, g));
    const neg_graph G = neg_graph_of(s, g);
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * GM_NEG_THREADS, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out, GM_EINVAL, "%s: NULL argument", what);
    hipLaunchKernelGGL(k_has_edges, dim3((unsigned)((n + GM_NEG_THREADS - 1) / GM_NEG_THREADS)), dim3(GM_NEG_THREADS), 0, (hipStream_t)stream, G, d_pairs, n, d_out);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
