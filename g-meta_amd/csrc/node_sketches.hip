// ELPH / BUDDY neighbourhood sketches of every node of a parent graph (gm_store_sketch_build, gm_sketch_*; the DEFINITION is in include/gmeta_hip.h,
// tests/sketch_ref.py restates it): per node and level d = 0 .. H a HyperLogLog record of 2^p one-byte registers and a MinHash record of K words of its
// d-hop ball, and the pair kernel that turns 2 (H + 1) records into the integers the estimators are made of.
//   layout      level-major, then node-major: sk[level][node][RD dwords], RD = 2^p / 4 + K: the HLL registers four to a dword (register j is byte j of the
//               record), the K MinHash words behind them.  A record is one contiguous run of 144 .. 3,072 bytes.  Level 0 is STORED (k_sketch_init).
//   a level     k_sketch_level: a wave per (row, chunk of 64 dwords), the lanes across the chunk's dwords, so a neighbour costs one coalesced 256-byte read
//               per chunk; GM_SK_UNROLL neighbours' loads are in flight.  The HLL dwords fold by byte-wise max, the MinHash dwords by u32 min; the row's own
//               record of the level before is folded in and the dword stored once.  max and min are idempotent and commutative: neither the order of a row
//               nor where it is cut can change a bit.
//   hub rows    rows of more than C entries (gm_set_tuning("sketch_chunk"); gm_columns.h: gm_col_hub_cut) are left out of that launch: k_sketch_parts folds
//               every segment of C entries into a partial record in scratch, k_sketch_hubs folds a row's partials and its own record.  No atomics.
//   pairs       k_sketch_pairs<H + 1>: a wave per pair reads the 2 (H + 1) records once, chunk by chunk, and forms the (H + 1)^2 combinations: the matches as
//               popcounts of ballots, the zero registers and the sum of 2^(32 - register) of the element-wise max in ONE 64-bit integer per lane (sk_term)
//               reduced by shuffles; the finished entries go through LDS to plain vector stores of consecutive int64.  No atomics, no floats.
//   features    k_sketch_pair_features<H + 1>: the same counting body (sk_pair_tab, ONE copy for both kernels), then the estimators of the header in fp64 in the
//               same wave -- a lane per entry, a lane per cell, the cells through LDS -- and (H + 2)^2 consecutive float32 stores per pair.  No atomics.
// A build runs on the caller's stream and is complete on the device when it returns; the sketch is read-only afterwards and holds no pointer into the store.
#include "gm_columns.h"
#include "gm_devutil.h"

#define GM_SK_THREADS 256
#define GM_SK_WAVES (GM_SK_THREADS / GM_WAVE)
#define GM_SK_UNROLL 8                    // neighbours' record loads in flight per lane
#define GM_SK_CHUNK 256                   // the library's sketch_chunk: entries per segment of a hub row
#define GM_SK_MIB 8192                    // the library's sketch_mib: 8 GiB per build
#define GM_SK_SALT_HLL 0x534B4831         // 'SKH1'
#define GM_SK_SALT_MH 0x534B4D31          // 'SKM1'

struct gm_sketch {
    int64_t N = 0, bytes = 0;
    int32_t hops = 0, p = 0, k = 0;
    uint32_t* d = nullptr;                // [hops + 1][N][RD]
};

// m4 HLL dwords then K MinHash dwords = RD dwords per record, in NCH chunks of 64
struct sk_shape { int32_t m4, K, RD, NCH; };
static inline sk_shape sk_shape_of(int32_t p, int32_t k) {
    const int32_t m4 = (1 << p) / 4, RD = m4 + k;
    return {m4, k, RD, (RD + GM_WAVE - 1) / GM_WAVE};
}

// byte-wise max of two dwords whose bytes are below 128 (a register is at most 33 - p <= 29): byte i of (a | 0x80..) - b keeps its top bit exactly where
// a_i >= b_i, and no borrow crosses a byte
__device__ __forceinline__ uint32_t sk_bmax(uint32_t a, uint32_t b) {
    const uint32_t ge = (((a | 0x80808080u) - b) >> 7) & 0x01010101u;
    const uint32_t keep = ge * 0xFFu;
    return (a & keep) | (b & ~keep);
}
__device__ __forceinline__ uint32_t sk_fold(uint32_t a, uint32_t b, bool hll) { return hll ? sk_bmax(a, b) : (a < b ? a : b); }

// acc folded with dword `at` of the records of row[0 .. len) (P = level + at; row and len wave-uniform)
__device__ __forceinline__ uint32_t sk_fold_row(uint32_t acc, const int32_t* __restrict__ row, int32_t len, const uint32_t* __restrict__ P, int64_t RD, bool hll) {
    int32_t i = 0;
    for (; i + GM_SK_UNROLL <= len; i += GM_SK_UNROLL) {
        int32_t z[GM_SK_UNROLL]; uint32_t q[GM_SK_UNROLL];
#pragma unroll
        for (int k = 0; k < GM_SK_UNROLL; ++k) z[k] = row[i + k];
#pragma unroll
        for (int k = 0; k < GM_SK_UNROLL; ++k) q[k] = P[(int64_t)z[k] * RD];
#pragma unroll
        for (int k = 0; k < GM_SK_UNROLL; ++k) acc = sk_fold(acc, q[k], hll);
    }
    for (; i < len; ++i) acc = sk_fold(acc, P[(int64_t)row[i] * RD], hll);
    return acc;
}

// level 0: the record of {v}.  A thread per dword
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_init(int64_t N, sk_shape sh, int32_t p, uint32_t s_h, uint32_t s_m, uint32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * GM_SK_THREADS + threadIdx.x;
    if (t >= N * sh.RD) return;
    const uint32_t v = (uint32_t)(t / sh.RD);
    const int32_t d = (int32_t)(t % sh.RD);
    uint32_t val;
    if (d < sh.m4) {
        const uint32_t h = lowbias32(v ^ s_h), j = h >> (32 - p), w = h << p;
        const uint32_t rho = w ? (uint32_t)__clz((int)w) + 1u : (uint32_t)(33 - p);
        val = (int32_t)(j >> 2) == d ? rho << (8 * (j & 3)) : 0u;
    } else {
        val = lowbias32(lowbias32(v ^ s_m) + (uint32_t)(d - sh.m4 + 1) * 0x9E3779B9u);
    }
    out[t] = val;
}

// the wave's work item and its lane's dword: item = blockIdx * waves + wave (wave-uniform), dword = 64 (item % NCH) + lane, clamped into the record so that
// every lane runs the same loads (live: the lane owns a dword)
struct sk_item { int64_t it; int32_t d; bool live, hll; };
__device__ __forceinline__ sk_item sk_item_of(const sk_shape& sh) {
    const int32_t lane = (int32_t)threadIdx.x & (GM_WAVE - 1);
    const int32_t w = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x / GM_WAVE);
    const int64_t item = (int64_t)blockIdx.x * GM_SK_WAVES + w;
    const int32_t d = (int32_t)(item % sh.NCH) * GM_WAVE + lane;
    sk_item r;
    r.it = item / sh.NCH; r.live = d < sh.RD; r.d = r.live ? d : sh.RD - 1; r.hll = r.d < sh.m4;
    return r;
}

// prev -> next for the rows of at most C entries
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_level(gm_nbr_graph G, int32_t C, sk_shape sh, const uint32_t* __restrict__ prev, uint32_t* __restrict__ next) {
    const sk_item w = sk_item_of(sh);
    if (w.it >= G.N) return;
    const int64_t r0 = G.ptr[w.it], deg = G.ptr[w.it + 1] - r0;
    if (deg > C) return;
    const int64_t at = w.it * sh.RD + w.d;
    const uint32_t acc = sk_fold_row(prev[at], G.idx + r0, (int32_t)deg, prev + w.d, sh.RD, w.hll);
    if (w.live) next[at] = acc;
}

// part[item] = the fold of segment it_seg[item] of hub row it_row[item] (the identity: no register, no smaller word)
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_parts(gm_nbr_graph G, int32_t C, sk_shape sh, const int32_t* __restrict__ it_row, const int32_t* __restrict__ it_seg,
                                                                int64_t n_items, const uint32_t* __restrict__ prev, uint32_t* __restrict__ part) {
    const sk_item w = sk_item_of(sh);
    if (w.it >= n_items) return;
    const int32_t v = it_row[w.it];
    const int64_t r0 = G.ptr[v], beg = (int64_t)it_seg[w.it] * C;
    const int64_t left = G.ptr[v + 1] - r0 - beg;
    const int32_t len = (int32_t)(left < C ? left : C);
    const uint32_t acc = sk_fold_row(w.hll ? 0u : ~0u, G.idx + r0 + beg, len, prev + w.d, sh.RD, w.hll);
    if (w.live) part[w.it * sh.RD + w.d] = acc;
}

// a hub row: its own record of the level before folded with its segments' partials
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_hubs(sk_shape sh, const int32_t* __restrict__ hub_row, const int32_t* __restrict__ hub_first, int64_t n_hubs,
                                                               const uint32_t* __restrict__ prev, const uint32_t* __restrict__ part, uint32_t* __restrict__ next) {
    const sk_item w = sk_item_of(sh);
    if (w.it >= n_hubs) return;
    const int32_t v = hub_row[w.it], first = hub_first[w.it], segs = hub_first[w.it + 1] - first;
    const int64_t at = (int64_t)v * sh.RD + w.d;
    uint32_t acc = prev[at];
    for (int32_t k = 0; k < segs; ++k) acc = sk_fold(acc, part[(int64_t)(first + k) * sh.RD + w.d], w.hll);
    if (w.live) next[at] = acc;
}

// gm_sketch_registers: a thread per register byte and per MinHash word of an output row
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_read(const uint32_t* __restrict__ level, int64_t N, sk_shape sh, const int32_t* __restrict__ nodes, int64_t m,
                                                               uint8_t* __restrict__ hll, uint32_t* __restrict__ mh) {
    const int32_t mreg = sh.m4 * 4, per = mreg + sh.K;
    const int64_t t = (int64_t)blockIdx.x * GM_SK_THREADS + threadIdx.x;
    if (t >= m * per) return;
    const int64_t i = t / per;
    const int32_t e = (int32_t)(t % per), v = nodes[i];
    const bool in = v >= 0 && v < N;
    const uint32_t* rec = level + (int64_t)(in ? v : 0) * sh.RD;
    if (e < mreg) hll[i * mreg + e] = in ? (uint8_t)(rec[e >> 2] >> (8 * (e & 3))) : (uint8_t)0;
    else mh[i * sh.K + (e - mreg)] = in ? rec[sh.m4 + (e - mreg)] : 0u;
}

// what a register dword adds to a pair's 64-bit sum: 2^(32 - register) over its four bytes in the low 48 bits (a whole record stays below 2^43) and its zero
// bytes counted from bit 48 (at most 2^10 per record): one accumulator and one wave reduction carry both
#define GM_SK_ZERO_SHIFT 48
__device__ __forceinline__ uint64_t sk_term(uint32_t x) {
    const uint32_t zero = (uint32_t)((x & 0xFFu) == 0) + (uint32_t)((x & 0xFF00u) == 0) + (uint32_t)((x & 0xFF0000u) == 0) + (uint32_t)((x & 0xFF000000u) == 0);
    return (1ull << (32 - (x & 0xFFu))) + (1ull << (32 - ((x >> 8) & 0xFFu))) + (1ull << (32 - ((x >> 16) & 0xFFu))) + (1ull << (32 - (x >> 24))) + ((uint64_t)zero << GM_SK_ZERO_SHIFT);
}
__device__ __forceinline__ uint64_t sk_wave_sum(uint64_t x) {
#pragma unroll
    for (int o = GM_WAVE / 2; o > 0; o >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, o, GM_WAVE);
    return x;
}

// one wave's LDS hand-over between its lanes: the wave's LDS operations issue in order, so nothing waits; the fences and the barrier keep the compiler from
// moving an LDS access across the point
__device__ __forceinline__ void sk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tab[0 .. E) = [L1, L1, 3] (match, zeros, zsum) of the canonical pair's records at the levels (a, b); tab[E .. E + EB) = [2, L1, 2] (zeros, zsum) of u's, then v's,
// own records; all zeros for a node outside the graph.  The whole wave calls it (pa, pb wave-uniform); the entries are in the wave's LDS row when it returns
template <int L1>
__device__ __forceinline__ void sk_pair_tab(const uint32_t* __restrict__ sk, int64_t N, const sk_shape& sh, int32_t pa, int32_t pb, int32_t lane, int64_t* tab) {
    constexpr int E = L1 * L1 * 3, EB = 2 * L1 * 2;
    if (pa < 0 || pa >= N || pb < 0 || pb >= N) {                              // (wave-uniform)
        for (int i = lane; i < E + EB; i += GM_WAVE) tab[i] = 0;
        sk_wave_sync();
        return;
    }
    const int64_t u = pa < pb ? pa : pb, v = pa < pb ? pb : pa;
    const int64_t level = N * sh.RD;
    int32_t match[L1][L1];
    uint64_t zs[L1][L1], bs[2][L1];                                            // sk_term sums: of the unions, of the two nodes' own records
#pragma unroll
    for (int a = 0; a < L1; ++a) {
        bs[0][a] = 0; bs[1][a] = 0;
#pragma unroll
        for (int b = 0; b < L1; ++b) { match[a][b] = 0; zs[a][b] = 0; }
    }
    for (int32_t c = 0; c < sh.NCH; ++c) {
        const int32_t d = c * GM_WAVE + lane;
        const bool live = d < sh.RD;
        const int32_t dd = live ? d : sh.RD - 1;
        uint32_t ru[L1], rv[L1];
#pragma unroll
        for (int a = 0; a < L1; ++a) { ru[a] = sk[a * level + u * sh.RD + dd]; rv[a] = sk[a * level + v * sh.RD + dd]; }
        if (c * GM_WAVE < sh.m4) {                                             // the chunk holds registers (wave-uniform)
            const bool hl = live && d < sh.m4;
#pragma unroll
            for (int a = 0; a < L1; ++a) {
                bs[0][a] += hl ? sk_term(ru[a]) : 0ull;
                bs[1][a] += hl ? sk_term(rv[a]) : 0ull;
#pragma unroll
                for (int b = 0; b < L1; ++b) zs[a][b] += hl ? sk_term(sk_bmax(ru[a], rv[b])) : 0ull;
            }
        }
        if ((c + 1) * GM_WAVE > sh.m4) {                                       // ... MinHash words
            const bool mh = live && d >= sh.m4;
#pragma unroll
            for (int a = 0; a < L1; ++a)
#pragma unroll
                for (int b = 0; b < L1; ++b) match[a][b] += __popcll(__ballot(mh && ru[a] == rv[b]));
        }
    }
#pragma unroll
    for (int a = 0; a < L1; ++a) {
#pragma unroll
        for (int b = 0; b < L1; ++b) {
            const uint64_t s = sk_wave_sum(zs[a][b]);
            if (lane == 0) {
                tab[(a * L1 + b) * 3] = match[a][b];
                tab[(a * L1 + b) * 3 + 1] = (int64_t)(s >> GM_SK_ZERO_SHIFT); tab[(a * L1 + b) * 3 + 2] = (int64_t)(s & ((1ull << GM_SK_ZERO_SHIFT) - 1));
            }
        }
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint64_t s = sk_wave_sum(bs[side][a]);
            if (lane == 0) { tab[E + (side * L1 + a) * 2] = (int64_t)(s >> GM_SK_ZERO_SHIFT); tab[E + (side * L1 + a) * 2 + 1] = (int64_t)(s & ((1ull << GM_SK_ZERO_SHIFT) - 1)); }
        }
    }
    sk_wave_sync();                                                            // (lane 0's entries ahead of the wave's loads)
}

// out[e, L1, L1, 3], balls[e, 2, L1, 2] = the pair's entries as sk_pair_tab leaves them
template <int L1>
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_pairs(const uint32_t* __restrict__ sk, int64_t N, sk_shape sh, const int32_t* __restrict__ pairs, int64_t n,
                                                                int64_t* __restrict__ out, int64_t* __restrict__ balls) {
    constexpr int E = L1 * L1 * 3, EB = 2 * L1 * 2;
    __shared__ int64_t tab[GM_SK_WAVES][E + EB];
    const int32_t lane = (int32_t)threadIdx.x & (GM_WAVE - 1);
    const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x / GM_WAVE);
    const int64_t e = (int64_t)blockIdx.x * GM_SK_WAVES + wave;
    if (e >= n) return;                                                        // (a whole wave; no barrier below)
    int64_t* o = out + e * E;
    int64_t* ob = balls + e * EB;
    sk_pair_tab<L1>(sk, N, sh, pairs[2 * e], pairs[2 * e + 1], lane, tab[wave]);
    for (int i = lane; i < E; i += GM_WAVE) o[i] = tab[wave][i];
    for (int i = lane; i < EB; i += GM_WAVE) ob[i] = tab[wave][E + i];
}

// the HyperLogLog estimate of (zeros, zsum) at m = 2^p registers (include/gmeta_hip.h: card); every operation rounded once, in the header's order
__device__ __forceinline__ double sk_card(int64_t zeros, int64_t zsum, double m, double alpha) {
#pragma clang fp contract(off)
    const double z = (double)zeros, s = (double)zsum / 4294967296.0;
    if (!(s > 0.0)) return 0.0;
    const double est = alpha * m * m / s;
    return (est <= 2.5 * m && z > 0.0) ? m * log(m / z) : est;
}

// out[e * ld + 0 .. S) = the S = (L1 + 1)^2 structure columns of pair e (include/gmeta_hip.h: gm_sketch_pair_features), fp64 up to the final cast.  After the
// counts a lane per entry forms the L1^2 intersections and the 2 L1 ball sizes, a lane per cell the table -- inner cells, then the last row and column, then
// the corner, each phase reading the one before from the wave's LDS row -- and a lane per cell T and its column
template <int L1>
__global__ void __launch_bounds__(GM_SK_THREADS) k_sketch_pair_features(const uint32_t* __restrict__ sk, int64_t N, sk_shape sh, const int32_t* __restrict__ pairs, int64_t n,
                                                                        int32_t symmetric, double m, double alpha, float* __restrict__ out, int64_t ld) {
#pragma clang fp contract(off)
    constexpr int E = L1 * L1 * 3, EB = 2 * L1 * 2, NC = L1 * L1, NB = 2 * L1, W = L1 + 1, S = W * W;
    static_assert(NC + NB <= GM_WAVE && S <= GM_WAVE, "a lane per entry and per cell");
    __shared__ int64_t tab[GM_SK_WAVES][E + EB];
    __shared__ double est[GM_SK_WAVES][NC + NB];                               // C[a][b], then |B_a(u)|, then |B_a(v)|
    __shared__ double cell[GM_SK_WAVES][S];
    const int32_t lane = (int32_t)threadIdx.x & (GM_WAVE - 1);
    const int32_t wave = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.x / GM_WAVE);
    const int64_t e = (int64_t)blockIdx.x * GM_SK_WAVES + wave;
    if (e >= n) return;                                                        // (a whole wave; no barrier below)
    const int32_t pa = pairs[2 * e], pb = pairs[2 * e + 1];
    sk_pair_tab<L1>(sk, N, sh, pa, pb, lane, tab[wave]);
    const int64_t* t = tab[wave];
    double* C = est[wave];
    double* P = cell[wave];
    if (lane < NC) C[lane] = (double)t[lane * 3] / (double)sh.K * sk_card(t[lane * 3 + 1], t[lane * 3 + 2], m, alpha);
    else if (lane < NC + NB) C[lane] = sk_card(t[E + (lane - NC) * 2], t[E + (lane - NC) * 2 + 1], m, alpha);
    sk_wave_sync();
    const int32_t a = lane / W, b = lane % W;                                  // the lane's cell
    if (lane < S && a < L1 && b < L1) {                                        // the 2-D difference, along a first
        const double up = a ? C[(a - 1) * L1 + b] : 0.0, left = b ? C[a * L1 + b - 1] : 0.0, diag = a && b ? C[(a - 1) * L1 + b - 1] : 0.0;
        P[lane] = (C[a * L1 + b] - up) - (left - diag);
    }
    sk_wave_sync();
    if (lane < S && (a == L1) != (b == L1)) {                                  // the ring of the ball minus the inner row / column
        const int32_t side = a == L1, i = side ? b : a;
        const double ring = C[NC + side * L1 + i] - (i ? C[NC + side * L1 + i - 1] : 0.0);
        double sum = 0.0;
        for (int j = 0; j < L1; ++j) sum = sum + (side ? P[j * W + i] : P[i * W + j]);
        P[lane] = ring - sum;
    }
    sk_wave_sync();
    if (lane == S - 1) {                                                       // the corner: every table sums to N
        double sum = 0.0;
        for (int j = 0; j < S - 1; ++j) sum = sum + P[j];
        P[lane] = (double)N - sum;
    }
    sk_wave_sync();
    if (lane < S) {
        const double own = P[lane], other = P[b * W + a];
        const double T = symmetric ? own + other : (pa <= pb ? own : other);
        out[e * ld + lane] = (float)log1p(T > 0.0 ? T : 0.0);
    }
}

// ---------------------------------------------------------------------------------------------------- host
static inline unsigned sk_grid(int64_t waves) { return (unsigned)((waves + GM_SK_WAVES - 1) / GM_SK_WAVES); }

extern "C" void gm_sketch_destroy(gm_sketch_t* sk) {
    if (!sk) return;
    if (sk->d) (void)hipFree(sk->d);                                           // (waits for the device: no kernel still reads the records)
    delete sk;
}

extern "C" int32_t gm_store_sketch_build(const gm_store_t* s, int32_t g, int32_t hops, int32_t p, int32_t k, uint64_t seed, void* stream, gm_sketch_t** out) {
    const char* what = "gm_store_sketch_build";
    GM_TRY(gm_store_call_check(what, s, g));
    GM_REQUIRE(out, GM_EINVAL, "%s: out is NULL", what);
    *out = nullptr;
    GM_REQUIRE(hops >= 1 && hops <= 4, GM_EINVAL, "%s: hops = %d; 1 .. 4", what, hops);
    GM_REQUIRE(p >= 4 && p <= 10, GM_EINVAL, "%s: p = %d; 4 .. 10", what, p);
    GM_REQUIRE(k >= 32 && k <= 512 && k % 32 == 0, GM_EINVAL, "%s: k = %d; a multiple of 32 in 32 .. 512", what, k);
    const int chunk = gm_knob().sketch_chunk, mib = gm_knob().sketch_mib;
    GM_REQUIRE(chunk >= 0, GM_EINVAL, "%s: sketch_chunk = %d", what, chunk);
    GM_REQUIRE(mib >= 0, GM_EINVAL, "%s: sketch_mib = %d", what, mib);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t N = s->node_off[g + 1] - s->node_off[g];
    const sk_shape sh = sk_shape_of(p, k);
    const int64_t level = N * sh.RD, bytes = (int64_t)(hops + 1) * level * (int64_t)sizeof(uint32_t), budget = (int64_t)(mib ? mib : GM_SK_MIB) << 20;
    GM_REQUIRE(bytes <= budget, GM_ERANGE, "%s: the sketches take %lld bytes at N = %lld, hops = %d, p = %d, k = %d; sketch_mib = %d holds %lld", what, (long long)bytes,
               (long long)N, hops, p, k, mib ? mib : GM_SK_MIB, (long long)budget);
    GM_REQUIRE((N * sh.NCH + GM_SK_WAVES - 1) / GM_SK_WAVES <= (int64_t)INT32_MAX && (level + GM_SK_THREADS - 1) / GM_SK_THREADS <= (int64_t)INT32_MAX, GM_ERANGE,
               "%s: %lld nodes of %d dwords pass the launch's 2^31 workgroups", what, (long long)N, sh.RD);
    GM_TRY(gm_nbr_index(s));
    const gm_nbr_graph G = gm_nbr_graph_of(s, g);
    const int32_t C = chunk ? chunk : GM_SK_CHUNK;

    struct guard { gm_sketch* sk; ~guard() { gm_sketch_destroy(sk); } } own = {new gm_sketch};
    gm_sketch* sk = own.sk;
    sk->N = N; sk->bytes = bytes; sk->hops = hops; sk->p = p; sk->k = k;
    GM_HIP(hipMalloc((void**)&sk->d, (size_t)(bytes ? bytes : 4)));
    if (N) {
        gm_stager sg(st);
        gm_scratch sc(st);
        const int64_t* h_ptr = sg.download(G.ptr, (size_t)(N + 1));
        GM_REQUIRE(h_ptr, GM_ENOMEM, "%s: pinned staging allocation failed", what);
        GM_HIP(hipStreamSynchronize(st));
        gm_col_hub_lists hl;
        GM_TRY(gm_col_hub_cut(what, h_ptr, N, C, 25, "sketch_chunk", &hl));
        gm_col_hubs<uint32_t> H;
        GM_TRY(gm_col_hubs_put(&H, hl, sh.RD, sc, sg));
        const dim3 block(GM_SK_THREADS);
        hipLaunchKernelGGL(k_sketch_init, dim3((unsigned)((level + GM_SK_THREADS - 1) / GM_SK_THREADS)), block, 0, st, N, sh, p, sample_salt(seed, g, GM_SK_SALT_HLL, 0),
                           sample_salt(seed, g, GM_SK_SALT_MH, 0), sk->d);
        GM_HIP(hipGetLastError());
        gm_phase_timer tm(what);
        if (tm.on) { GM_HIP(hipStreamSynchronize(st)); tm.lap("level 0"); }
        for (int32_t d = 1; d <= hops; ++d) {
            const uint32_t* prev = sk->d + (int64_t)(d - 1) * level;
            uint32_t* next = sk->d + (int64_t)d * level;
            hipLaunchKernelGGL(k_sketch_level, dim3(sk_grid(N * sh.NCH)), block, 0, st, G, C, sh, prev, next);
            if (H.n_hubs) {
                hipLaunchKernelGGL(k_sketch_parts, dim3(sk_grid(H.n_items * sh.NCH)), block, 0, st, G, C, sh, (const int32_t*)H.it_row, (const int32_t*)H.it_seg, H.n_items, prev, H.part);
                hipLaunchKernelGGL(k_sketch_hubs, dim3(sk_grid(H.n_hubs * sh.NCH)), block, 0, st, sh, (const int32_t*)H.row, (const int32_t*)H.first, H.n_hubs, prev,
                                   (const uint32_t*)H.part, next);
            }
            GM_HIP(hipGetLastError());
            if (tm.on) { GM_HIP(hipStreamSynchronize(st)); tm.lap("level"); }
        }
        GM_HIP(hipStreamSynchronize(st));                                      // complete on the device: afterwards any stream reads the records without an event
    }
    own.sk = nullptr;
    *out = sk;
    return GM_OK;
}

extern "C" int32_t gm_sketch_dims(const gm_sketch_t* sk, int64_t* n_nodes, int32_t* hops, int32_t* p, int32_t* k, int64_t* bytes) {
    GM_REQUIRE(sk, GM_EINVAL, "gm_sketch_dims: sketch is NULL");
    if (n_nodes) *n_nodes = sk->N;
    if (hops) *hops = sk->hops;
    if (p) *p = sk->p;
    if (k) *k = sk->k;
    if (bytes) *bytes = sk->bytes;
    return GM_OK;
}

extern "C" int32_t gm_sketch_registers(const gm_sketch_t* sk, int32_t level, const int32_t* d_nodes, int64_t m, uint8_t* d_hll, uint32_t* d_minhash, void* stream) {
    const char* what = "gm_sketch_registers";
    GM_REQUIRE(sk, GM_EINVAL, "%s: sketch is NULL", what);
    GM_REQUIRE(level >= 0 && level <= sk->hops, GM_EINVAL, "%s: level = %d of a sketch with hops = %d", what, level, sk->hops);
    GM_REQUIRE(m >= 0 && m <= (int64_t)INT32_MAX, GM_EINVAL, "%s: m = %lld", what, (long long)m);
    if (m == 0) return GM_OK;
    GM_REQUIRE(d_nodes && d_hll && d_minhash, GM_EINVAL, "%s: NULL argument", what);
    const sk_shape sh = sk_shape_of(sk->p, sk->k);
    const int64_t threads = m * (4 * sh.m4 + sh.K);
    hipLaunchKernelGGL(k_sketch_read, dim3((unsigned)((threads + GM_SK_THREADS - 1) / GM_SK_THREADS)), dim3(GM_SK_THREADS), 0, (hipStream_t)stream,
                       (const uint32_t*)sk->d + (int64_t)level * sk->N * sh.RD, sk->N, sh, d_nodes, m, d_hll, d_minhash);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

template <int L1>
static void sk_pairs(hipStream_t st, const gm_sketch* sk, const sk_shape& sh, const int32_t* d_pairs, int64_t n, int64_t* d_out, int64_t* d_out_balls) {
    hipLaunchKernelGGL(k_sketch_pairs<L1>, dim3(sk_grid(n)), dim3(GM_SK_THREADS), 0, st, (const uint32_t*)sk->d, sk->N, sh, d_pairs, n, d_out, d_out_balls);
}

extern "C" int32_t gm_sketch_pair_counts(const gm_sketch_t* sk, const int32_t* d_pairs, int64_t n, int64_t* d_out, int64_t* d_out_balls, void* stream) {
    const char* what = "gm_sketch_pair_counts";
    GM_REQUIRE(sk, GM_EINVAL, "%s: sketch is NULL", what);
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out && d_out_balls, GM_EINVAL, "%s: NULL argument", what);
    const sk_shape sh = sk_shape_of(sk->p, sk->k);
    const hipStream_t st = (hipStream_t)stream;
    switch (sk->hops) {
        case 1: sk_pairs<2>(st, sk, sh, d_pairs, n, d_out, d_out_balls); break;
        case 2: sk_pairs<3>(st, sk, sh, d_pairs, n, d_out, d_out_balls); break;
        case 3: sk_pairs<4>(st, sk, sh, d_pairs, n, d_out, d_out_balls); break;
        default: sk_pairs<5>(st, sk, sh, d_pairs, n, d_out, d_out_balls); break;
    }
    GM_HIP(hipGetLastError());
    return GM_OK;
}

template <int L1>
static void sk_pair_features(hipStream_t st, const gm_sketch* sk, const sk_shape& sh, const int32_t* d_pairs, int64_t n, int32_t symmetric, double m, double alpha,
                             float* d_out, int64_t ld) {
    hipLaunchKernelGGL(k_sketch_pair_features<L1>, dim3(sk_grid(n)), dim3(GM_SK_THREADS), 0, st, (const uint32_t*)sk->d, sk->N, sh, d_pairs, n, symmetric, m, alpha, d_out, ld);
}

extern "C" int32_t gm_sketch_pair_features(const gm_sketch_t* sk, const int32_t* d_pairs, int64_t n, int32_t symmetric, float* d_out, int64_t ld, void* stream) {
    const char* what = "gm_sketch_pair_features";
    GM_REQUIRE(sk, GM_EINVAL, "%s: sketch is NULL", what);
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    const int32_t S = (sk->hops + 2) * (sk->hops + 2);
    GM_REQUIRE(ld >= S, GM_EINVAL, "%s: ld = %lld; at least (hops + 2)^2 = %d", what, (long long)ld, S);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out, GM_EINVAL, "%s: NULL argument", what);
    const sk_shape sh = sk_shape_of(sk->p, sk->k);
    const hipStream_t st = (hipStream_t)stream;
    const int32_t regs = 1 << sk->p;
    const double m = (double)regs;                                             // alpha as gmeta_amd.hll_cardinality forms it
    const double alpha = regs == 16 ? 0.673 : regs == 32 ? 0.697 : regs == 64 ? 0.709 : 0.7213 / (1.0 + 1.079 / m);
    switch (sk->hops) {
        case 1: sk_pair_features<2>(st, sk, sh, d_pairs, n, symmetric, m, alpha, d_out, ld); break;
        case 2: sk_pair_features<3>(st, sk, sh, d_pairs, n, symmetric, m, alpha, d_out, ld); break;
        case 3: sk_pair_features<4>(st, sk, sh, d_pairs, n, symmetric, m, alpha, d_out, ld); break;
        default: sk_pair_features<5>(st, sk, sh, d_pairs, n, symmetric, m, alpha, d_out, ld); break;
    }
    GM_HIP(hipGetLastError());
    return GM_OK;
}
