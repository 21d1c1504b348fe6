// Rank counts of positive scores against negative scores, and their reduction to the integers and the one double behind Hits@K, MRR and AUC
// (gm_rank_counts / gm_rank_summary).  The DEFINITION -- order, ranges, counts, summary, errors -- is in include/gmeta_hip.h; tests/ranking_ref.py restates it
// by direct comparison and the GPU tests compare integer for integer.  This file is how it is computed:
//   k_rank_keys     one thread per score: the order-preserving uint32 key (-0 -> +0, then the sign fold), the NaN check, and per positive the range check; a
//                   range longer than RK_CUT is appended to a list (an integer atomic counter: the list's ORDER may differ from run to run, what is counted
//                   for its members cannot).  Every later kernel reads the flag word first and does nothing where it is set: a bad range is never walked.
//   ranged mode     k_rank_ranged: a wave per positive sweeps its range with coalesced loads (ranges up to RK_CUT);
//                   k_rank_long: a fixed grid walks the list; chunk c of the list's entry l belongs to workgroup (c + l) mod grid, integer atomics combine.
//   shared mode     brute force (k_rank_brute): a thread per positive, tiles of the negatives' keys in LDS read as broadcast 16-byte words, the slices of the
//                   negatives combined with integer atomics;
//                   sorted: a keys-only LSD radix sort of the N keys, 8 bits a pass -- k_rank_hist (per-workgroup digit counts, digit-major), a two-level
//                   exclusive scan over (digit, workgroup) (k_rank_scan_local / k_rank_scan_top, on the workgroup scan of the candidate selection), and
//                   k_rank_scatter (stable: a wave ranks its keys by ballot match against per-wave digit counters, waves in order) -- then k_rank_search:
//                   a lower-bound and an upper-bound binary search per positive.
//                   Which of the two runs: gm_set_tuning("rank_sort_min") / GM_RANK_SORT_MIN, else rk_sorts(); the integers are the same.
//   summary         k_rank_partial: fixed ranges of RK_SUM_RANGE positives -> {rr, auc2, n_pairs, hits}; k_rank_final adds the partials: the integers in any
//                   order, rr by one wave -- lane l the partials l, l + 64, ... ascending, then a fixed shuffle tree: no float atomics, the same bits for the same inputs.
// Everything runs on the caller's stream; keys, sort buffers, list and partials are ONE block from the stream-ordered pool that goes back to it on that stream.  The
// host reads one record (flag words + summary) once, behind everything.
#include "gm_internal.h"

#define RK_THREADS 256
#define RK_WAVES (RK_THREADS / GM_WAVE)
#define RK_CUT 4096                       // ranges longer than this leave the wave sweep for k_rank_long
#define RK_LONG_GRID 1024
#define RK_LONG_CHUNK (RK_THREADS * 8)
#define RK_TILE 2048                      // keys of the negatives per LDS tile of k_rank_brute
#define RK_SORT_ITEMS 16
#define RK_SORT_TILE (RK_THREADS * RK_SORT_ITEMS)
#define RK_SCAN_ITEMS 8
#define RK_SCAN_TILE (RK_THREADS * RK_SCAN_ITEMS)
#define RK_SUM_RANGE 1024
#define RK_F_NAN_POS 1
#define RK_F_NAN_NEG 2
#define RK_F_RANGE 4

static_assert(RK_THREADS == GM_CAND_THREADS, "the scans run on gm_cand_scan");

// what the host reads back (zeroed by one memset): info[0] the RK_F_* bits, info[1 .. 3] the largest ~index, hence the smallest index, of a NaN positive / a NaN
// negative / a bad range; n_long: the length of the list of long ranges
struct rk_record { unsigned long long info[4]; gm_rank_summary_t sum; int32_t n_long, pad; };
struct rk_ks { int64_t k[GM_RANK_MAX_K]; int32_t n; };
struct rk_partial { double rr; int64_t auc2, n_pairs, hits[GM_RANK_MAX_K]; };

__device__ __forceinline__ uint32_t rk_key(uint32_t u) {
    if (u == 0x80000000u) u = 0u;                                              // -0.0 == +0.0
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ bool rk_nan(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

__global__ void __launch_bounds__(RK_THREADS)
k_rank_keys(const uint32_t* __restrict__ pos, int64_t P, const uint32_t* __restrict__ neg, int64_t N, const int64_t* __restrict__ range, uint32_t* __restrict__ kp,
            uint32_t* __restrict__ kn, unsigned long long* info, int32_t* __restrict__ long_list, int32_t* n_long) {
    const int64_t t = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
    if (t < P) {
        const uint32_t u = pos[t];
        if (rk_nan(u)) { atomicOr(&info[0], (unsigned long long)RK_F_NAN_POS); atomicMax(&info[1], ~(unsigned long long)t); }
        kp[t] = rk_key(u);
        if (range) {
            const int64_t b = range[2 * t], e = range[2 * t + 1];
            if (b < 0 || e < b || e > N) { atomicOr(&info[0], (unsigned long long)RK_F_RANGE); atomicMax(&info[3], ~(unsigned long long)t); }
            else if (e - b > RK_CUT) long_list[atomicAdd(n_long, 1)] = (int32_t)t;
        }
    } else if (t - P < N) {
        const int64_t j = t - P;
        const uint32_t u = neg[j];
        if (rk_nan(u)) { atomicOr(&info[0], (unsigned long long)RK_F_NAN_NEG); atomicMax(&info[2], ~(unsigned long long)j); }
        kn[j] = rk_key(u);
    }
}

__device__ __forceinline__ int rk_wave_sum(int v) {
#pragma unroll
    for (int o = GM_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GM_WAVE);
    return v;
}

// ---- ranged mode.  counts was zeroed: a long range's pair is left to k_rank_long
__global__ void __launch_bounds__(RK_THREADS)
k_rank_ranged(const uint32_t* __restrict__ kp, int64_t P, const uint32_t* __restrict__ kn, const int64_t* __restrict__ range, const unsigned long long* info,
              int64_t* __restrict__ counts) {
    if (info[0]) return;
    const int lane = (int)threadIdx.x & (GM_WAVE - 1);
    const int64_t i = (int64_t)blockIdx.x * RK_WAVES + threadIdx.x / GM_WAVE;
    if (i >= P) return;
    const int64_t b = range[2 * i], e = range[2 * i + 1];
    if (e - b > RK_CUT) return;
    const uint32_t key = kp[i];
    int gt = 0, eq = 0;
    int64_t j = b + lane;
    for (; j + 3 * GM_WAVE < e; j += 4 * GM_WAVE) {                            // four loads in flight
        const uint32_t a0 = kn[j], a1 = kn[j + GM_WAVE], a2 = kn[j + 2 * GM_WAVE], a3 = kn[j + 3 * GM_WAVE];
        gt += (a0 > key) + (a1 > key) + (a2 > key) + (a3 > key);
        eq += (a0 == key) + (a1 == key) + (a2 == key) + (a3 == key);
    }
    for (; j < e; j += GM_WAVE) { const uint32_t a = kn[j]; gt += a > key; eq += a == key; }
    gt = rk_wave_sum(gt); eq = rk_wave_sum(eq);
    if (lane == 0) { counts[2 * i] = gt; counts[2 * i + 1] = eq; }
}

// sums of gt / eq over the workgroup -> thread 0 (lds: 2 * RK_WAVES ints)
__device__ __forceinline__ void rk_block_sum(int& gt, int& eq, int* lds) {
    gt = rk_wave_sum(gt); eq = rk_wave_sum(eq);
    const int lane = (int)threadIdx.x & (GM_WAVE - 1), wave = (int)threadIdx.x / GM_WAVE;
    __syncthreads();
    if (lane == 0) { lds[2 * wave] = gt; lds[2 * wave + 1] = eq; }
    __syncthreads();
    if (threadIdx.x == 0) { gt = 0; eq = 0; for (int w = 0; w < RK_WAVES; ++w) { gt += lds[2 * w]; eq += lds[2 * w + 1]; } }
}

__global__ void __launch_bounds__(RK_THREADS)
k_rank_long(const uint32_t* __restrict__ kp, const uint32_t* __restrict__ kn, const int64_t* __restrict__ range, const unsigned long long* info,
            const int32_t* __restrict__ long_list, const int32_t* n_long, int64_t* counts) {
    __shared__ int lds[2 * RK_WAVES];
    if (info[0]) return;
    const int n = *n_long, G = (int)gridDim.x, g = (int)blockIdx.x;
    for (int l = 0; l < n; ++l) {
        const int32_t i = long_list[l];
        const int64_t b = range[2 * (int64_t)i], e = range[2 * (int64_t)i + 1];
        int64_t c = (int64_t)(((g - l) % G + G) % G);                          // chunk c belongs to workgroup (c + l) mod G
        if (b + c * RK_LONG_CHUNK >= e) continue;                              // (uniform over the workgroup)
        const uint32_t key = kp[i];
        int gt = 0, eq = 0;
        for (; b + c * RK_LONG_CHUNK < e; c += G) {
            const int64_t j0 = b + c * RK_LONG_CHUNK, j1 = j0 + RK_LONG_CHUNK < e ? j0 + RK_LONG_CHUNK : e;
            for (int64_t j = j0 + threadIdx.x; j < j1; j += RK_THREADS) { const uint32_t a = kn[j]; gt += a > key; eq += a == key; }
        }
        rk_block_sum(gt, eq, lds);
        if (threadIdx.x == 0) {
            if (gt) atomicAdd((unsigned long long*)&counts[2 * (int64_t)i], (unsigned long long)gt);
            if (eq) atomicAdd((unsigned long long*)&counts[2 * (int64_t)i + 1], (unsigned long long)eq);
        }
    }
}

// ---- shared mode, brute force.  counts was zeroed; blockIdx.y walks the tiles y, y + gridDim.y, ...
__global__ void __launch_bounds__(RK_THREADS)
k_rank_brute(const uint32_t* __restrict__ kp, int64_t P, const uint32_t* __restrict__ kn, int64_t N, const unsigned long long* info, int64_t* counts) {
    __shared__ uint4 tile[RK_TILE / 4];
    if (info[0]) return;
    const int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
    const uint32_t key = i < P ? kp[i] : 0u;
    long long gt = 0, eq = 0;
    uint32_t* t32 = (uint32_t*)tile;
    for (int64_t j0 = (int64_t)blockIdx.y * RK_TILE; j0 < N; j0 += (int64_t)gridDim.y * RK_TILE) {
        const int cnt = (int)(N - j0 < RK_TILE ? N - j0 : RK_TILE);
        __syncthreads();                                                       // (the previous tile's readers are through)
        for (int q = (int)threadIdx.x; q < cnt; q += RK_THREADS) t32[q] = kn[j0 + q];
        __syncthreads();
        int g = 0, s = 0;
        const int full = cnt >> 2;
        for (int q = 0; q < full; ++q) {                                       // every lane reads the same 16 bytes: a broadcast
            const uint4 a = tile[q];
            g += (a.x > key) + (a.y > key) + (a.z > key) + (a.w > key);
            s += (a.x == key) + (a.y == key) + (a.z == key) + (a.w == key);
        }
        for (int q = full << 2; q < cnt; ++q) { const uint32_t a = t32[q]; g += a > key; s += a == key; }
        gt += g; eq += s;
    }
    if (i < P) {
        if (gt) atomicAdd((unsigned long long*)&counts[2 * i], (unsigned long long)gt);
        if (eq) atomicAdd((unsigned long long*)&counts[2 * i + 1], (unsigned long long)eq);
    }
}

// ---- shared mode, sorted: the radix sort of the negatives' keys
// the lanes of the wave that hold the same digit as this one (valid lanes only)
__device__ __forceinline__ unsigned long long rk_peers(uint32_t d, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// hist[d * nb + workgroup]: keys of the workgroup's tile whose digit is d
__global__ void __launch_bounds__(RK_THREADS) k_rank_hist(const uint32_t* __restrict__ keys, int64_t n, int shift, int32_t nb, int32_t* __restrict__ hist) {
    __shared__ int cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = (int)threadIdx.x & (GM_WAVE - 1), wave = (int)threadIdx.x / GM_WAVE;
    const int64_t base = (int64_t)blockIdx.x * RK_SORT_TILE + wave * (GM_WAVE * RK_SORT_ITEMS) + lane;
#pragma unroll 4
    for (int j = 0; j < RK_SORT_ITEMS; ++j) {
        const int64_t idx = base + j * GM_WAVE;
        const bool valid = idx < n;
        const uint32_t d = valid ? (keys[idx] >> shift) & 255u : 0u;
        const unsigned long long m = rk_peers(d, valid);
        if (valid && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&cnt[d], __popcll(m));      // the lowest lane of the group adds for it
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * nb + blockIdx.x] = cnt[threadIdx.x];
}

// x[0 .. m) -> exclusive prefix inside tiles of RK_SCAN_TILE, in place; sums[tile] = the tile's total
__global__ void __launch_bounds__(RK_THREADS) k_rank_scan_local(int32_t* __restrict__ x, int64_t m, int32_t* __restrict__ sums) {
    __shared__ int part[GM_CAND_WAVES];
    const int64_t base = (int64_t)blockIdx.x * RK_SCAN_TILE + (int64_t)threadIdx.x * RK_SCAN_ITEMS;
    int v[RK_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < RK_SCAN_ITEMS; ++j) { v[j] = base + j < m ? x[base + j] : 0; s += v[j]; }
    int total;
    int run = gm_cand_scan(s, part, &total) - s;
#pragma unroll
    for (int j = 0; j < RK_SCAN_ITEMS; ++j) { if (base + j < m) x[base + j] = run; run += v[j]; }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. n) -> exclusive prefix, in place (one workgroup)
__global__ void __launch_bounds__(RK_THREADS) k_rank_scan_top(int32_t* __restrict__ sums, int32_t n) {
    __shared__ int part[GM_CAND_WAVES];
    int carry = 0;
    for (int32_t b0 = 0; b0 < n; b0 += RK_THREADS) {
        const int32_t b = b0 + (int32_t)threadIdx.x;
        const int v = b < n ? sums[b] : 0;
        int total;
        const int inc = gm_cand_scan(v, part, &total);
        if (b < n) sums[b] = carry + inc - v;
        carry += total;
    }
}

// in -> out, stable by the digit.  Order inside a tile: wave, then round j, then lane -- the order of the indices
__global__ void __launch_bounds__(RK_THREADS)
k_rank_scatter(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t n, int shift, int32_t nb, const int32_t* __restrict__ hist, const int32_t* __restrict__ sums) {
    __shared__ int cnt_s[RK_WAVES][256];
    for (int w = 0; w < RK_WAVES; ++w) cnt_s[w][threadIdx.x] = 0;
    __syncthreads();
    const int lane = (int)threadIdx.x & (GM_WAVE - 1), wave = (int)threadIdx.x / GM_WAVE;
    volatile int* cnt = cnt_s[wave];                                           // this wave's row: written by one lane per digit and round, in program order
    const int64_t base = (int64_t)blockIdx.x * RK_SORT_TILE + wave * (GM_WAVE * RK_SORT_ITEMS) + lane;
    uint32_t key[RK_SORT_ITEMS];
    int rank[RK_SORT_ITEMS];
#pragma unroll
    for (int j = 0; j < RK_SORT_ITEMS; ++j) {
        const int64_t idx = base + j * GM_WAVE;
        const bool valid = idx < n;
        key[j] = valid ? in[idx] : 0u;
        const uint32_t d = (key[j] >> shift) & 255u;
        const unsigned long long m = rk_peers(d, valid);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        const int seen = valid ? cnt[d] : 0;                                   // the group reads one address: before its lowest lane writes it
        rank[j] = seen + below;
        __builtin_amdgcn_wave_barrier();
        if (valid && below == 0) cnt[d] = seen + __popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // digit d = threadIdx.x: where the tile's keys of that digit start, then wave by wave
        const int64_t at = (int64_t)threadIdx.x * nb + blockIdx.x;
        int g = hist[at] + sums[at / RK_SCAN_TILE];
        for (int w = 0; w < RK_WAVES; ++w) { const int t = cnt_s[w][threadIdx.x]; cnt_s[w][threadIdx.x] = g; g += t; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RK_SORT_ITEMS; ++j) {
        const int64_t idx = base + j * GM_WAVE;
        if (idx < n) out[(int64_t)cnt_s[wave][(key[j] >> shift) & 255u] + rank[j]] = key[j];
    }
}

// ks[0 .. N) ascending: gt = N - (first index with a key above), eq = (that) - (first index with a key not below)
__global__ void __launch_bounds__(RK_THREADS)
k_rank_search(const uint32_t* __restrict__ kp, int64_t P, const uint32_t* __restrict__ ks, int64_t N, const unsigned long long* info, int64_t* __restrict__ counts) {
    if (info[0]) return;
    const int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
    if (i >= P) return;
    const uint32_t key = kp[i];
    int64_t lo = 0, hi = N;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (ks[mid] < key) lo = mid + 1; else hi = mid; }
    const int64_t lb = lo;
    hi = N;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (ks[mid] <= key) lo = mid + 1; else hi = mid; }
    counts[2 * i] = N - lo; counts[2 * i + 1] = lo - lb;
}

// ---- summary
__global__ void __launch_bounds__(RK_THREADS)
k_rank_partial(const int64_t* __restrict__ counts, int64_t P, int64_t N, const int64_t* __restrict__ range, rk_ks ks, const unsigned long long* info, rk_partial* __restrict__ part) {
    __shared__ double s_rr[RK_WAVES];
    __shared__ long long s_i[RK_WAVES][2 + GM_RANK_MAX_K];
    if (info[0]) return;
    double rr = 0.0;
    long long v[2 + GM_RANK_MAX_K];
#pragma unroll
    for (int q = 0; q < 2 + GM_RANK_MAX_K; ++q) v[q] = 0;
    const int64_t i0 = (int64_t)blockIdx.x * RK_SUM_RANGE + threadIdx.x;
#pragma unroll
    for (int j = 0; j < RK_SUM_RANGE / RK_THREADS; ++j) {
        const int64_t i = i0 + (int64_t)j * RK_THREADS;
        if (i >= P) break;
        const int64_t gt = counts[2 * i], eq = counts[2 * i + 1], Ni = range ? range[2 * i + 1] - range[2 * i] : N;
        rr += 1.0 / (1.0 + ((double)gt + 0.5 * (double)eq));
        v[0] += 2 * (Ni - gt - eq) + eq;
        v[1] += Ni;
#pragma unroll
        for (int q = 0; q < GM_RANK_MAX_K; ++q) v[2 + q] += (q < ks.n && gt + eq < ks.k[q]) ? 1 : 0;
    }
    const int lane = (int)threadIdx.x & (GM_WAVE - 1), wave = (int)threadIdx.x / GM_WAVE;
#pragma unroll
    for (int o = GM_WAVE / 2; o > 0; o >>= 1) {
        rr += __shfl_xor(rr, o, GM_WAVE);
#pragma unroll
        for (int q = 0; q < 2 + GM_RANK_MAX_K; ++q) v[q] += __shfl_xor(v[q], o, GM_WAVE);
    }
    if (lane == 0) {
        s_rr[wave] = rr;
#pragma unroll
        for (int q = 0; q < 2 + GM_RANK_MAX_K; ++q) s_i[wave][q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        rk_partial p;
        p.rr = 0.0; p.auc2 = 0; p.n_pairs = 0;
        for (int q = 0; q < GM_RANK_MAX_K; ++q) p.hits[q] = 0;
        for (int w = 0; w < RK_WAVES; ++w) {                                   // waves in ascending order
            p.rr += s_rr[w]; p.auc2 += s_i[w][0]; p.n_pairs += s_i[w][1];
            for (int q = 0; q < GM_RANK_MAX_K; ++q) p.hits[q] += s_i[w][2 + q];
        }
        part[blockIdx.x] = p;
    }
}

// one wave: lane l adds the partials l, l + 64, ... in ascending order, then a fixed tree
__global__ void __launch_bounds__(GM_WAVE) k_rank_final(const rk_partial* __restrict__ part, int64_t nb, int64_t P, rk_record* rec) {
    if (rec->info[0]) return;
    double rr = 0.0;
    long long v[2 + GM_RANK_MAX_K];
#pragma unroll
    for (int q = 0; q < 2 + GM_RANK_MAX_K; ++q) v[q] = 0;
    for (int64_t b = threadIdx.x; b < nb; b += GM_WAVE) {
        const rk_partial p = part[b];
        rr += p.rr; v[0] += p.auc2; v[1] += p.n_pairs;
#pragma unroll
        for (int q = 0; q < GM_RANK_MAX_K; ++q) v[2 + q] += p.hits[q];
    }
#pragma unroll
    for (int o = GM_WAVE / 2; o > 0; o >>= 1) {
        rr += __shfl_xor(rr, o, GM_WAVE);
#pragma unroll
        for (int q = 0; q < 2 + GM_RANK_MAX_K; ++q) v[q] += __shfl_xor(v[q], o, GM_WAVE);
    }
    if (threadIdx.x == 0) {
        rec->sum.n_pos = P; rec->sum.n_pairs = v[1]; rec->sum.auc2 = v[0]; rec->sum.rr_sum = rr;
        for (int q = 0; q < GM_RANK_MAX_K; ++q) rec->sum.hits[q] = v[2 + q];
    }
}

// ---- host side
// The library's own choice between the two shared-mode paths (rank_sort_min == 0).  The sort costs a fixed chain of eighteen small launches and a few sweeps of
// N keys; brute force costs rows * N comparisons, rows = P rounded up to the workgroup.  Measured (profiles/ranking.txt, the grid of tools/ranking_bench.py):
// brute force 0.08 ms up to rows * N = 2^24 and 0.10 ms at 2^28 against 0.14 - 0.19 ms sorted; 0.52 ms at 2^32 against 0.17 - 0.19: the cut is 2^30.
static bool rk_sorts(int64_t P, int64_t N) {
    const int64_t rows = (P + RK_THREADS - 1) / RK_THREADS * RK_THREADS;
    return N >= 4096 && rows * N >= ((int64_t)1 << 30);
}

static int rk_run(const char* what, const float* d_pos, int64_t P, const float* d_neg, int64_t N, const int64_t* d_range, const int64_t* h_ks, int32_t n_k,
                  int64_t* d_counts, gm_rank_summary_t* h_out, bool summary, hipStream_t st) {
    GM_REQUIRE(P >= 0 && P <= (int64_t)INT32_MAX, GM_EINVAL, "%s: P = %lld", what, (long long)P);
    GM_REQUIRE(N >= 0 && N <= (int64_t)INT32_MAX, GM_EINVAL, "%s: N = %lld", what, (long long)N);
    rk_ks ks;
    memset(&ks, 0, sizeof(ks));
    if (summary) {
        GM_REQUIRE(n_k >= 0 && n_k <= GM_RANK_MAX_K, GM_EINVAL, "%s: n_k = %d; 0 .. %d", what, n_k, GM_RANK_MAX_K);
        GM_REQUIRE(n_k == 0 || h_ks, GM_EINVAL, "%s: h_ks is NULL with n_k = %d", what, n_k);
        for (int j = 0; j < n_k; ++j) {
            GM_REQUIRE(h_ks[j] >= 1, GM_EINVAL, "%s: h_ks[%d] = %lld; a K is at least 1", what, j, (long long)h_ks[j]);
            ks.k[j] = h_ks[j];
        }
        ks.n = n_k;
        GM_REQUIRE(h_out, GM_EINVAL, "%s: h_out is NULL", what);
    }
    const int knob = gm_knob().rank_sort_min;
    GM_REQUIRE(knob >= 0, GM_EINVAL, "%s: rank_sort_min = %d", what, knob);
    if (P == 0) {
        if (summary) memset(h_out, 0, sizeof(*h_out));
        return GM_OK;
    }
    GM_REQUIRE(d_pos, GM_EINVAL, "%s: d_pos is NULL with P = %lld", what, (long long)P);
    GM_REQUIRE(d_neg || N == 0, GM_EINVAL, "%s: d_neg is NULL with N = %lld", what, (long long)N);
    GM_REQUIRE(summary || d_counts, GM_EINVAL, "%s: d_counts is NULL with P = %lld", what, (long long)P);
    GM_REQUIRE(P * N <= ((int64_t)1 << 61), GM_ERANGE, "%s: P = %lld positives against N = %lld negatives: n_pairs could pass 2^61", what, (long long)P, (long long)N);

    // one block of scratch for the whole call (an allocation from the stream-ordered pool costs the host 20 - 35 us: eight of them were as long as the kernels)
    const bool sorted = !d_range && N > 0 && (knob ? N >= knob : rk_sorts(P, N));
    const int32_t nb = (int32_t)((N + RK_SORT_TILE - 1) / RK_SORT_TILE);
    const int64_t m = (int64_t)256 * nb;
    const int32_t n_sums = (int32_t)((m + RK_SCAN_TILE - 1) / RK_SCAN_TILE);
    const int64_t nbp = (P + RK_SUM_RANGE - 1) / RK_SUM_RANGE;
    size_t total = 0;
    auto carve = [&total](size_t bytes) { const size_t at = total; total += (bytes + 255) / 256 * 256; return at; };
    const size_t o_rec = carve(sizeof(rk_record)), o_kp = carve((size_t)P * 4), o_kn = carve((size_t)N * 4), o_list = carve(d_range ? (size_t)P * 4 : 0),
                 o_cnt = carve(d_counts ? 0 : (size_t)P * 16), o_alt = carve(sorted ? (size_t)N * 4 : 0), o_hist = carve(sorted ? (size_t)m * 4 : 0),
                 o_sums = carve(sorted ? (size_t)n_sums * 4 : 0), o_part = carve(summary ? (size_t)nbp * sizeof(rk_partial) : 0);
    gm_scratch sc(st);
    char* base = nullptr;
    GM_TRY(sc.take(&base, total));
    rk_record* rec = (rk_record*)(base + o_rec);
    uint32_t *kp = (uint32_t*)(base + o_kp), *kn = (uint32_t*)(base + o_kn), *alt = (uint32_t*)(base + o_alt);
    int32_t *long_list = (int32_t*)(base + o_list), *n_long = &rec->n_long, *hist = (int32_t*)(base + o_hist), *sums = (int32_t*)(base + o_sums);
    rk_partial* part = (rk_partial*)(base + o_part);
    if (!d_counts) d_counts = (int64_t*)(base + o_cnt);
    GM_HIP(hipMemsetAsync(rec, 0, sizeof(*rec), st));
    if (!sorted) GM_HIP(hipMemsetAsync(d_counts, 0, (size_t)(2 * P) * sizeof(int64_t), st));      // (the search stores every pair; the sweeps add)
    gm_stager sg(st);
    rk_record* h_rec = (rk_record*)sg.take(sizeof(rk_record));
    GM_REQUIRE(h_rec, GM_ENOMEM, "%s: pinned staging allocation failed", what);

    gm_phase_timer tm("rank");                                                  // GM_TIMING: the stream is synchronised behind every phase
    auto lap = [&](const char* phase) { if (tm.on) { (void)hipStreamSynchronize(st); tm.lap(phase); } };
    const dim3 block(RK_THREADS);
    auto blocks = [](int64_t n, int64_t per) { return dim3((unsigned)((n + per - 1) / per)); };
    hipLaunchKernelGGL(k_rank_keys, blocks(P + N, RK_THREADS), block, 0, st, (const uint32_t*)d_pos, P, (const uint32_t*)d_neg, N, d_range, kp, kn, rec->info, long_list, n_long);
    lap("keys");
    if (d_range) {
        hipLaunchKernelGGL(k_rank_ranged, blocks(P, RK_WAVES), block, 0, st, (const uint32_t*)kp, P, (const uint32_t*)kn, d_range, (const unsigned long long*)rec->info, d_counts);
        hipLaunchKernelGGL(k_rank_long, dim3(RK_LONG_GRID), block, 0, st, (const uint32_t*)kp, (const uint32_t*)kn, d_range, (const unsigned long long*)rec->info,
                           (const int32_t*)long_list, (const int32_t*)n_long, d_counts);
        lap("sweep");
    } else if (sorted) {
        uint32_t *src = kn, *dst = alt;
        for (int shift = 0; shift < 32; shift += 8) {
            hipLaunchKernelGGL(k_rank_hist, dim3((unsigned)nb), block, 0, st, (const uint32_t*)src, N, shift, nb, hist);
            hipLaunchKernelGGL(k_rank_scan_local, dim3((unsigned)n_sums), block, 0, st, hist, m, sums);
            hipLaunchKernelGGL(k_rank_scan_top, dim3(1), block, 0, st, sums, n_sums);
            hipLaunchKernelGGL(k_rank_scatter, dim3((unsigned)nb), block, 0, st, (const uint32_t*)src, dst, N, shift, nb, (const int32_t*)hist, (const int32_t*)sums);
            std::swap(src, dst);
        }                                                                      // four passes: the sorted keys are back in kn
        lap("sort");
        hipLaunchKernelGGL(k_rank_search, blocks(P, RK_THREADS), block, 0, st, (const uint32_t*)kp, P, (const uint32_t*)src, N, (const unsigned long long*)rec->info, d_counts);
        lap("search");
    } else if (N > 0) {
        // slices of the negatives: enough workgroups to fill the device where the positives alone do not
        const int64_t bx = (P + RK_THREADS - 1) / RK_THREADS, tiles = (N + RK_TILE - 1) / RK_TILE;
        const int64_t by = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(tiles, 65535), (4096 + bx - 1) / bx));
        hipLaunchKernelGGL(k_rank_brute, dim3((unsigned)bx, (unsigned)by), block, 0, st, (const uint32_t*)kp, P, (const uint32_t*)kn, N, (const unsigned long long*)rec->info, d_counts);
        lap("sweep");
    }
    if (summary) {
        hipLaunchKernelGGL(k_rank_partial, dim3((unsigned)nbp), block, 0, st, (const int64_t*)d_counts, P, N, d_range, ks, (const unsigned long long*)rec->info, part);
        hipLaunchKernelGGL(k_rank_final, dim3(1), dim3(GM_WAVE), 0, st, (const rk_partial*)part, nbp, P, rec);
        lap("summary");
    }
    GM_HIP(hipGetLastError());
    GM_HIP(hipMemcpyAsync(h_rec, rec, sizeof(rk_record), hipMemcpyDeviceToHost, st));
    GM_HIP(hipStreamSynchronize(st));
    const unsigned long long f = h_rec->info[0];
    if (f & RK_F_RANGE) {
        const long long i = (long long)~h_rec->info[3];
        int64_t* h_r = (int64_t*)sg.take(2 * sizeof(int64_t));
        GM_REQUIRE(h_r, GM_ENOMEM, "%s: pinned staging allocation failed", what);
        GM_HIP(hipMemcpyAsync(h_r, d_range + 2 * i, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        GM_HIP(hipStreamSynchronize(st));
        GM_REQUIRE(false, GM_EINVAL, "%s: range %lld = (%lld, %lld) with N = %lld; 0 <= b <= e <= N", what, i, (long long)h_r[0], (long long)h_r[1], (long long)N);
    }
    GM_REQUIRE(!(f & RK_F_NAN_POS), GM_EINVAL, "%s: d_pos[%lld] is a NaN", what, (long long)~h_rec->info[1]);
    GM_REQUIRE(!(f & RK_F_NAN_NEG), GM_EINVAL, "%s: d_neg[%lld] is a NaN", what, (long long)~h_rec->info[2]);
    if (summary) *h_out = h_rec->sum;
    return GM_OK;
}

extern "C" int32_t gm_rank_counts(const float* d_pos, int64_t P, const float* d_neg, int64_t N, const int64_t* d_neg_range, int64_t* d_counts, void* stream) {
    return rk_run("gm_rank_counts", d_pos, P, d_neg, N, d_neg_range, nullptr, 0, d_counts, nullptr, false, (hipStream_t)stream);
}

extern "C" int32_t gm_rank_summary(const float* d_pos, int64_t P, const float* d_neg, int64_t N, const int64_t* d_neg_range, const int64_t* h_ks, int32_t n_k,
                                   int64_t* d_counts, gm_rank_summary_t* h_out, void* stream) {
    return rk_run("gm_rank_summary", d_pos, P, d_neg, N, d_neg_range, h_ks, n_k, d_counts, h_out, true, (hipStream_t)stream);
}
