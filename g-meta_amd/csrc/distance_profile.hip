// The joint hop-distance profile of node pairs (gm_store_pair_distance_profile; the DEFINITION is in include/gmeta_hip.h, tests/distance_profile_ref.py restates
// it): what the export in pair_distance.hip runs on the state of its search, so that only the [n, D + 2, D + 2] tables leave the device.
//   planes      the search (pair_distance.hip: dist_rounds) keeps ONE BIT per (node, column), a 64-bit word of `next` holding 64 columns of a node, and a bit
//               of next is set at exactly one level.  A pair's table counts nodes, so behind every level t = 0 .. D k_prof_transpose turns next[N, W] into the
//               plane T[t][column][ceil(N / 64)], where a word holds 64 NODES of a column.  A 64 x 64 bit tile is 64 ballots of a wave whose lanes hold the
//               words of 64 nodes: the ballot of bit b IS word b of the transposed tile.  A workgroup of 8 waves takes 8 tiles of nodes x 8 words of columns
//               (a lane reads 64 consecutive bytes of its node's row) and stages the 512 x 8 result words in LDS, rows padded to 9 words (ds_write_b64 of 16
//               consecutive lanes then meets 16 distinct bank pairs), so that a column's 8 consecutive node-words leave as one 64-byte segment.  The planes
//               are zeroed once per group of columns; a level that found no bit (flag 0), and a workgroup whose words are all 0, store nothing.  Nodes >= N
//               read as 0, so the tail bits of a column's last word stay 0; the padding columns of a group are never set by the search.
//   counting    k_prof_count<L>, L = D + 1: a wave per pair, its lanes striding over the node-words.  Per word the L plane words of the pair's two columns;
//               popc(Ta & Tb) into L x L int32 registers, popc(Ta) and popc(Tb) into the margins; a wave reduction; row and column D + 1 by subtraction
//               from the margins and from N.  No atomics: the finished table goes through LDS to plain vector stores of consecutive ints.  A duplicate pair
//               is an entry of its own reading the same columns.
// Everything runs on the caller's stream.
#include "gm_internal.h"

#define GM_PROF_WAVES 8                   // waves of a transposing workgroup = node tiles it takes
#define GM_PROF_WORDS 8                   // words of columns it takes: 64 consecutive bytes of a node's row
#define GM_PROF_LD (GM_PROF_WAVES + 1)    // words per LDS row (a column's node-words, padded)
#define GM_PROF_COUNT_THREADS 256

// next[N, W] -> plane[64 W, NW], NW = ceil(N / 64).  Workgroup (wg, jg): words wg * 8 .. + 8 of the nodes 512 jg .. + 512
__global__ void __launch_bounds__(GM_PROF_WAVES * GM_WAVE) k_prof_transpose(const uint64_t* __restrict__ next, int32_t W, int64_t N, int64_t NW, int32_t w_groups,
                                                                            const int32_t* __restrict__ flag, uint64_t* __restrict__ plane) {
    __shared__ uint64_t tile[GM_PROF_WORDS * GM_WAVE * GM_PROF_LD];
    if (flag[0] == 0) return;
    const int32_t lane = (int32_t)threadIdx.x & (GM_WAVE - 1), wave = (int32_t)threadIdx.x / GM_WAVE;
    const int32_t w0 = (int32_t)(blockIdx.x % (unsigned)w_groups) * GM_PROF_WORDS;
    const int64_t j0 = (int64_t)(blockIdx.x / (unsigned)w_groups) * GM_PROF_WAVES;
    const int64_t v = (j0 + wave) * GM_WAVE + lane;
    uint64_t word[GM_PROF_WORDS];
    bool any = false;
#pragma unroll
    for (int k = 0; k < GM_PROF_WORDS; ++k) {
        word[k] = v < N && w0 + k < W ? next[v * W + w0 + k] : 0ull;
        any |= word[k] != 0;
    }
    if (!__syncthreads_or(any)) return;                                        // (the planes were zeroed)
    // A ballot is wave-uniform and lane b keeps ballot b.  The lanes b mod 8 == i take it with one AND-OR against sel[i] (all ones on those lanes), and
    // the lanes b / 8 == o keep what the eight ballots of their octet left: four vector instructions per ballot.  (The empty asm keeps sel[i] a register:
    // as a compare the compiler folds it into selects that read two scalar operands each, a move more per ballot.)
    uint32_t sel[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sel[i] = (lane & 7) == i ? ~0u : 0u;
        asm volatile("" : "+v"(sel[i]));
    }
#pragma unroll
    for (int k = 0; k < GM_PROF_WORDS; ++k) {
        const uint32_t half[2] = {(uint32_t)word[k], (uint32_t)(word[k] >> 32)};
        uint32_t lo = 0, hi = 0;                                               // lane b: word b of the transposed tile
#pragma unroll
        for (int o = 0; o < GM_WAVE / 8; ++o) {
            uint32_t tl = 0, th = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int b = o * 8 + i;
                const uint64_t col = __ballot((half[b >> 5] & (1u << (b & 31))) != 0);      // the nodes of this tile that hold column 64 (w0 + k) + b
                tl |= (uint32_t)col & sel[i];
                th |= (uint32_t)(col >> 32) & sel[i];
            }
            const bool mine = (lane >> 3) == o;
            lo = mine ? tl : lo;
            hi = mine ? th : hi;
        }
        tile[(k * GM_WAVE + lane) * GM_PROF_LD + wave] = ((uint64_t)hi << 32) | lo;
    }
    __syncthreads();
    const int32_t jj = (int32_t)threadIdx.x % GM_PROF_WAVES, c = (int32_t)threadIdx.x / GM_PROF_WAVES;      // 8 consecutive threads: one column's 64 bytes
    if (j0 + jj >= NW) return;
#pragma unroll
    for (int k = 0; k < GM_PROF_WORDS; ++k) {
        if (w0 + k >= W) break;
        plane[((int64_t)(w0 + k) * GM_WAVE + c) * NW + j0 + jj] = tile[(k * GM_WAVE + c) * GM_PROF_LD + jj];
    }
}

__device__ __forceinline__ int32_t prof_wave_sum(int32_t x) {
#pragma unroll
    for (int o = GM_WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, GM_WAVE);
    return x;
}

// T[L, B, NW]: the planes of a group of B columns.  Entry e of the group: the columns cu[e], cv[e] of its pair -> out[dst[e], L + 1, L + 1]
template <int L>
__global__ void __launch_bounds__(GM_PROF_COUNT_THREADS) k_prof_count(const uint64_t* __restrict__ T, int64_t B, int64_t N, int64_t NW, const int32_t* __restrict__ cu,
                                                                      const int32_t* __restrict__ cv, const int64_t* __restrict__ dst, int64_t cnt, int32_t* __restrict__ out) {
    constexpr int S = L + 1, E = S * S;                                        // the table's side and entries
    __shared__ int32_t tab[GM_PROF_COUNT_THREADS / GM_WAVE][E];
    const int32_t lane = (int32_t)threadIdx.x & (GM_WAVE - 1), wave = (int32_t)threadIdx.x / GM_WAVE;
    const int64_t e = (int64_t)blockIdx.x * (GM_PROF_COUNT_THREADS / GM_WAVE) + wave;
    if (e >= cnt) return;                                                      // (a whole wave; no barrier below)
    const uint64_t* Tu = T + (int64_t)cu[e] * NW;
    const uint64_t* Tv = T + (int64_t)cv[e] * NW;
    const int64_t level = B * NW;
    int32_t acc[L][L], mu[L], mv[L];
#pragma unroll
    for (int a = 0; a < L; ++a) {
        mu[a] = 0; mv[a] = 0;
#pragma unroll
        for (int b = 0; b < L; ++b) acc[a][b] = 0;
    }
    for (int64_t j = lane; j < NW; j += GM_WAVE) {
        uint64_t ta[L], tb[L];
#pragma unroll
        for (int a = 0; a < L; ++a) { ta[a] = Tu[a * level + j]; tb[a] = Tv[a * level + j]; }
#pragma unroll
        for (int a = 0; a < L; ++a) {
            mu[a] += __popcll(ta[a]); mv[a] += __popcll(tb[a]);
#pragma unroll
            for (int b = 0; b < L; ++b) acc[a][b] += __popcll(ta[a] & tb[b]);
        }
    }
    int32_t rest = (int32_t)N;                                                 // N - everything else: P[D + 1][D + 1]
    int32_t far_v[L];                                                          // P[D + 1][b]
#pragma unroll
    for (int b = 0; b < L; ++b) far_v[b] = prof_wave_sum(mv[b]);
#pragma unroll
    for (int a = 0; a < L; ++a) {
        int32_t far_u = prof_wave_sum(mu[a]);                                  // P[a][D + 1]
#pragma unroll
        for (int b = 0; b < L; ++b) {
            const int32_t p = prof_wave_sum(acc[a][b]);
            far_u -= p; far_v[b] -= p; rest -= p;
            if (lane == 0) tab[wave][a * S + b] = p;
        }
        rest -= far_u;
        if (lane == 0) tab[wave][a * S + L] = far_u;
    }
#pragma unroll
    for (int b = 0; b < L; ++b) {
        rest -= far_v[b];
        if (lane == 0) tab[wave][L * S + b] = far_v[b];
    }
    if (lane == 0) tab[wave][E - 1] = rest;
    __builtin_amdgcn_wave_barrier();                                           // (lane 0's LDS stores are ordered ahead of the wave's loads: one wave, in order)
    int32_t* o = out + dst[e] * E;
    for (int i = lane; i < E; i += GM_WAVE) o[i] = tab[wave][i];
}

int gm_prof_transpose(hipStream_t st, const uint64_t* next, int32_t W, int64_t N, const int32_t* flag, uint64_t* plane) {
    const int64_t NW = (N + GM_WAVE - 1) / GM_WAVE;
    const int32_t w_groups = (W + GM_PROF_WORDS - 1) / GM_PROF_WORDS;
    const int64_t blocks = (NW + GM_PROF_WAVES - 1) / GM_PROF_WAVES * w_groups;
    GM_REQUIRE(blocks <= (int64_t)INT32_MAX, GM_ERANGE, "gm_store_pair_distance_profile: %lld transposing workgroups in one level", (long long)blocks);
    hipLaunchKernelGGL(k_prof_transpose, dim3((unsigned)blocks), dim3(GM_PROF_WAVES * GM_WAVE), 0, st, next, W, N, NW, w_groups, flag, plane);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

template <int L>
static void prof_count(hipStream_t st, const uint64_t* T, int64_t B, int64_t N, const int32_t* cu, const int32_t* cv, const int64_t* dst, int64_t cnt, int32_t* out) {
    const int per = GM_PROF_COUNT_THREADS / GM_WAVE;
    hipLaunchKernelGGL(k_prof_count<L>, dim3((unsigned)((cnt + per - 1) / per)), dim3(GM_PROF_COUNT_THREADS), 0, st, T, B, N, (N + GM_WAVE - 1) / GM_WAVE, cu, cv, dst, cnt, out);
}

int gm_prof_count(hipStream_t st, const uint64_t* T, int32_t D, int64_t B, int64_t N, const int32_t* cu, const int32_t* cv, const int64_t* dst, int64_t cnt, int32_t* out) {
    if (!cnt) return GM_OK;
    switch (D) {
        case 1: prof_count<2>(st, T, B, N, cu, cv, dst, cnt, out); break;
        case 2: prof_count<3>(st, T, B, N, cu, cv, dst, cnt, out); break;
        case 3: prof_count<4>(st, T, B, N, cu, cv, dst, cnt, out); break;
        case 4: prof_count<5>(st, T, B, N, cu, cv, dst, cnt, out); break;
        case 5: prof_count<6>(st, T, B, N, cu, cv, dst, cnt, out); break;
        case 6: prof_count<7>(st, T, B, N, cu, cv, dst, cnt, out); break;
        case 7: prof_count<8>(st, T, B, N, cu, cv, dst, cnt, out); break;
        default: GM_REQUIRE(false, GM_EINVAL, "gm_store_pair_distance_profile: max_dist = %d; 1 .. 7", D);
    }
    GM_HIP(hipGetLastError());
    return GM_OK;
}
