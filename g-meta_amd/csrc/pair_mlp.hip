// The BUDDY pair predictor on the hop-propagated levels (gm_prop_pair_mlp_*; the DEFINITION is in include/gmeta_hip.h, tests/pair_mlp_ref.py restates it):
//   z_k = [ op(x_t[a], x_t[b]) for t = 0 .. hops | s_k ],  h_k = relu(z_k W1 + b1),  l_k = h_k . w2 + b2,  the BCE-with-logits loss and all its gradients.
// The [n, K] matrix Z never stands in memory: both GEMMs form their Z operand in LDS from gathers of the level rows.
//   forward     k_pmlp_fwd<STEP>: a workgroup of 4 waves takes PM_T = 128 pairs and walks K in chunks of PM_KC = 16 columns, level by level (a chunk never straddles two
//               levels; the tail chunk of a level and of the structure columns is zero-filled), then the structure columns.  A thread gathers 8 columns of both rows
//               of one pair as two 16-byte loads each, forms op ONCE in fp32 (the operation of k_prop_pairs) and writes the chunk k-major to LDS beside the chunk's
//               W1 rows.  Two LDS images: the next chunk's loads are issued before the current chunk's MFMAs and written to the other image behind them, one barrier
//               per chunk; two workgroups per CU (the launch bound keeps the kernel within 256 registers).  Wave w owns the hidden columns [64 w, 64 w + 64): 4 x 2
//               blocks of v_mfma_f32_32x32x2_f32, K order = chunk order, ascending inside a chunk -- the same for every row of every tile.
//   epilogue    + b1, relu, * w2 in registers; a row's columns are added as (column j, column j + 32) per lane, a butterfly over the 32 lanes, then the four waves in
//               ascending order, + b2.  STEP: the loss term and dl_k of every row, dh = dl w2 [h > 0] stored to scratch ([rows, HP], HP = Hd padded to 64), and the
//               tile's column sums of dl h (dw2), of dh (db1), of dl (db2) and of the loss terms: rows ascending per lane, lower half + upper half, to scratch.
//   wgrad       k_pmlp_wgrad: dW1 = Z^T dH.  grid (K tiles of 64 rows of W1, row ranges); a workgroup re-gathers and re-forms its 64 columns of z for 32 pairs per
//               stage (row-major in LDS: the transposed operand is a conflict-free read), loads the pairs' dh rows, and runs 2 x 2 blocks per wave.  Partials
//               [range][K][Hd] go to scratch.
//   reduce      k_pmlp_reduce: a thread per parameter adds the ranges' (dW1) or tiles' (b1, w2, b2, loss) partials in ascending order and, from the second chunk of a
//               step on, adds the chunk's sum to the running value.  No atomics.
// A step walks n in chunks of pair_mlp_rows pairs (the dh scratch's budget); ranges are PM_RANGE rows, or a 256th of the call's largest chunk where that is more.
#include "gm_internal.h"

typedef float pm_f16 __attribute__((ext_vector_type(16)));

#define PM_THREADS 256
#define PM_T 128                          // pairs per forward tile
#define PM_KC 16                          // z columns per forward chunk
#define PM_ZLD (PM_T + 1)                 // forward Zs [2][PM_KC][PM_ZLD], k-major
#define PM_WLD (256 + 4)                  // Ws [2][PM_KC][PM_WLD] / wgrad Ds [PM_WR][PM_WLD]
#define PM_WK 64                          // rows of W1 per weight-gradient tile
#define PM_WR 32                          // pairs per weight-gradient stage
#define PM_WZLD (PM_WK + 4)               // wgrad Zs [PM_WR][PM_WZLD], row-major
#define PM_RANGE 1024                     // pairs per weight-gradient range (at least)
#define PM_MAX_RANGES 256
#define PM_ROWS 65536                     // the library's pair_mlp_rows
#define PM_MAX_HD 256
#define PM_MAX_S 256

struct pm_args {
    const float* x; int64_t N; int32_t L1, F, ld;            // the levels
    const int32_t* pairs; const float* extra; int32_t S;      // the chunk's pairs / structure columns (already offset), n of them
    int64_t n;
    int32_t op, K, Hd, HP;
    const float *W1, *b1, *w2, *b2;
};

__device__ __forceinline__ float pm_op(int32_t op, float a, float b) { return op == GM_PROP_HADAMARD ? a * b : fabsf(a - b); }

// the 8 z values of one pair at the level columns f .. f + 7 of level rows pa / pb (NULL: a pair without rows); columns from ld on are zero
__device__ __forceinline__ void pm_gather8(const float* __restrict__ pa, const float* __restrict__ pb, int32_t f, int32_t ld, float4 (&qa)[2], float4 (&qb)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        qa[h] = make_float4(0.f, 0.f, 0.f, 0.f); qb[h] = qa[h];
        if (pa && f + 4 * h + 4 <= ld) { qa[h] = *(const float4*)(pa + f + 4 * h); qb[h] = *(const float4*)(pb + f + 4 * h); }
    }
}
__device__ __forceinline__ void pm_form8(int32_t op, const float4 (&qa)[2], const float4 (&qb)[2], float (&z)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        z[4 * h + 0] = pm_op(op, qa[h].x, qb[h].x); z[4 * h + 1] = pm_op(op, qa[h].y, qb[h].y);
        z[4 * h + 2] = pm_op(op, qa[h].z, qb[h].z); z[4 * h + 3] = pm_op(op, qa[h].w, qb[h].w);
    }
}
// 8 structure columns s .. s + 7 of a row of `extra` (NULL: none); columns from S on are zero
__device__ __forceinline__ void pm_extra8(const float* __restrict__ row, int32_t s, int32_t S, float4 (&qa)[2]) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = row && s + j < S ? row[s + j] : 0.f;
    qa[0] = make_float4(v[0], v[1], v[2], v[3]); qa[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// ---------------------------------------------------------------------------------------------------- forward (+ loss, dl, dh and the tile's column sums)
// tile partials of a step: tp[tile][2 HP + 4] = dw2 [HP] | db1 [HP] | db2 | loss | - | -
template <bool STEP>
__global__ void __launch_bounds__(PM_THREADS, 2) k_pmlp_fwd(pm_args A, const float* __restrict__ labels, float inv_scale_n, float* __restrict__ logits, float* __restrict__ dh,
                                                         float* __restrict__ tp) {
    __shared__ float Zs[2][PM_KC * PM_ZLD];
    __shared__ float Ws[2][PM_KC * PM_WLD];
    __shared__ float red[4 * PM_T];
    __shared__ float dls[PM_T];
    __shared__ float tsum[4];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int32_t w = __builtin_amdgcn_readfirstlane(tid >> 6), cb = w * 64;
    const bool active = cb < A.HP;
    const int64_t row0 = (int64_t)blockIdx.x * PM_T;
    // the thread's pair: tile row tid / 2, 8 columns from (tid % 2) * 8 of a chunk
    const int32_t gr = tid >> 1, gq = (tid & 1) * 8;
    const float *pa = nullptr, *pb = nullptr, *pe = nullptr;
    {
        const int64_t r = row0 + gr;
        if (r < A.n) {
            const int32_t a = A.pairs[2 * r], b = A.pairs[2 * r + 1];
            if (a >= 0 && a < A.N && b >= 0 && b < A.N) { pa = A.x + (int64_t)a * A.ld; pb = A.x + (int64_t)b * A.ld; }
            if (A.S) pe = A.extra + r * A.S;
        }
    }
    const int32_t cpl = (A.F + PM_KC - 1) / PM_KC, nlev = A.L1 * cpl, nch = nlev + (A.S + PM_KC - 1) / PM_KC;
    const int64_t level = A.N * A.ld;

    float4 qa[2], qb[2];
    float wv[PM_KC];
    auto load = [&](int32_t c) {
        int32_t kbase, f0, lim;                                                  // W1 rows kbase + k for k < lim are the chunk's
        if (c < nlev) {
            const int32_t t = c / cpl;
            f0 = (c - t * cpl) * PM_KC; kbase = t * A.F + f0; lim = A.F - f0;
            pm_gather8(pa ? pa + t * level : nullptr, pb ? pb + t * level : nullptr, f0 + gq, A.ld, qa, qb);
        } else {
            f0 = (c - nlev) * PM_KC; kbase = A.L1 * A.F + f0; lim = A.S - f0;
            pm_extra8(pe, f0 + gq, A.S, qa);
        }
#pragma unroll
        for (int k = 0; k < PM_KC; ++k) wv[k] = (tid < A.Hd && k < lim) ? A.W1[(int64_t)(kbase + k) * A.Hd + tid] : 0.f;
    };
    auto store = [&](int32_t c) {
        float* Z = Zs[c & 1];
        float* W = Ws[c & 1];
        float z[8];
        if (c < nlev) pm_form8(A.op, qa, qb, z);
        else { z[0] = qa[0].x; z[1] = qa[0].y; z[2] = qa[0].z; z[3] = qa[0].w; z[4] = qa[1].x; z[5] = qa[1].y; z[6] = qa[1].z; z[7] = qa[1].w; }
#pragma unroll
        for (int j = 0; j < 8; ++j) Z[(gq + j) * PM_ZLD + gr] = z[j];
#pragma unroll
        for (int k = 0; k < PM_KC; ++k) W[k * PM_WLD + tid] = wv[k];
    };

    pm_f16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // two LDS images: chunk c + 1 is written while the MFMAs of chunk c drain, one barrier per chunk
    if (nch > 0) { load(0); store(0); }
    __syncthreads();
    for (int32_t c = 0; c < nch; ++c) {
        if (c + 1 < nch) load(c + 1);
        if (active) {
            const float* Z = Zs[c & 1];
            const float* W = Ws[c & 1];
#pragma unroll 4
            for (int kk = 0; kk < PM_KC; kk += 2) {
                float av[4], bv[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = Z[(kk + half) * PM_ZLD + i * 32 + l31];
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = W[(kk + half) * PM_WLD + cb + j * 32 + l31];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        }
        if (c + 1 < nch) store(c + 1);                                           // the other image: last read before the previous barrier
        __syncthreads();
    }

    // C layout of the 32 x 32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    float b1v[2], w2v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t col = cb + j * 32 + l31;
        b1v[j] = col < A.Hd ? A.b1[col] : 0.f; w2v[j] = col < A.Hd ? A.w2[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float h0 = fmaxf(__fadd_rn(acc[i][0][e], b1v[0]), 0.f), h1 = fmaxf(__fadd_rn(acc[i][1][e], b1v[1]), 0.f);
            acc[i][0][e] = h0; acc[i][1][e] = h1;
            float s = __fmaf_rn(h1, w2v[1], __fmul_rn(h0, w2v[0]));             // (every rounding of a logit is spelled out: forward and step cannot contract differently)
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
            if (l31 == 0) red[w * PM_T + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * half] = s;
        }
    __syncthreads();
    if (tid < PM_T) {
        const float l = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(red[tid], red[PM_T + tid]), red[2 * PM_T + tid]), red[3 * PM_T + tid]), A.b2[0]);
        const int64_t r = row0 + tid;
        float dl = 0.f, term = 0.f;
        if (r < A.n) {
            if (logits) logits[r] = l;
            if (STEP) {
                const float y = labels[r], ex = expf(-fabsf(l)), sg = l >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
                dl = (sg - y) * inv_scale_n;
                term = ((fmaxf(l, 0.f) - l * y) + log1pf(ex)) * inv_scale_n;
            }
        }
        if (STEP) {
            dls[tid] = dl;
            float sd = dl, st = term;                                           // the tile's sums of dl and of the loss terms: a butterfly per wave, then wave 0 + wave 1
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { sd += __shfl_xor(sd, o, 64); st += __shfl_xor(st, o, 64); }
            if (lane == 0) { tsum[2 * w] = sd; tsum[2 * w + 1] = st; }
        }
    }
    if (!STEP) return;
    __syncthreads();
    float* tpt = tp + (int64_t)blockIdx.x * (2 * A.HP + 4);
    if (tid == 0) { tpt[2 * A.HP] = tsum[0] + tsum[2]; tpt[2 * A.HP + 1] = tsum[1] + tsum[3]; }
    if (!active) return;
    float sw[2] = {0.f, 0.f}, sb[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int32_t row = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
            const float dl = dls[row];                                          // 0 for the rows behind n
            const bool live = row0 + row < A.n;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float h = acc[i][j][e], d = (live && h > 0.f) ? dl * w2v[j] : 0.f;
                dh[(row0 + row) * A.HP + cb + j * 32 + l31] = d;                // (the scratch holds whole tiles: rows behind n are stored as zeros)
                sw[j] += live ? dl * h : 0.f; sb[j] += d;
            }
        }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        sw[j] += __shfl_xor(sw[j], 32, 64); sb[j] += __shfl_xor(sb[j], 32, 64);
        if (half == 0) { tpt[cb + j * 32 + l31] = sw[j]; tpt[A.HP + cb + j * 32 + l31] = sb[j]; }
    }
}

// ---------------------------------------------------------------------------------------------------- weight gradient
// part[range][K][Hd] = sum over the range's pairs, ascending, of z_k (x) dh_k, for the PM_WK rows of W1 of tile blockIdx.x.  rows_pad: the dh scratch's rows (whole tiles)
__global__ void __launch_bounds__(PM_THREADS) k_pmlp_wgrad(pm_args A, const float* __restrict__ dh, int64_t range_rows, int64_t rows_pad, float* __restrict__ part) {
    __shared__ float Zs[PM_WR * PM_WZLD];
    __shared__ float Ds[PM_WR * PM_WLD];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int32_t w = __builtin_amdgcn_readfirstlane(tid >> 6), cb = w * 64;
    const bool active = cb < A.HP;
    const int32_t tpl = (A.F + PM_WK - 1) / PM_WK, nlev = A.L1 * tpl, kt = (int32_t)blockIdx.x;
    const bool lev = kt < nlev;
    const int32_t t = lev ? kt / tpl : 0, f0 = lev ? (kt - t * tpl) * PM_WK : (kt - nlev) * PM_WK;
    const int32_t kbase = lev ? t * A.F + f0 : A.L1 * A.F + f0, lim = (lev ? A.F : A.S) - f0;     // W1 rows kbase + m, m < lim
    const float* xl = A.x + (int64_t)t * A.N * A.ld;
    const int64_t r_beg = (int64_t)blockIdx.y * range_rows, r_end = r_beg + range_rows < rows_pad ? r_beg + range_rows : rows_pad;
    const int32_t gr = tid >> 3, gq = (tid & 7) * 8;                             // the thread's pair of a stage and its 8 columns of the tile
    const int32_t dq = (tid & 7) * 32;                                          // its 32 columns of the pair's dh row

    float4 qa[2], qb[2], dv[8];
    auto load = [&](int64_t r0) {
        const int64_t r = r0 + gr;
        if (lev) {
            const float *pa = nullptr, *pb = nullptr;
            if (r < A.n) {
                const int32_t a = A.pairs[2 * r], b = A.pairs[2 * r + 1];
                if (a >= 0 && a < A.N && b >= 0 && b < A.N) { pa = xl + (int64_t)a * A.ld; pb = xl + (int64_t)b * A.ld; }
            }
            pm_gather8(pa, pb, f0 + gq, A.ld, qa, qb);
        } else pm_extra8(r < A.n ? A.extra + r * A.S : nullptr, f0 + gq, A.S, qa);
#pragma unroll
        for (int v = 0; v < 8; ++v) dv[v] = dq + 4 * v < A.HP ? *(const float4*)(dh + r * A.HP + dq + 4 * v) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store = [&]() {
        float z[8];
        if (lev) pm_form8(A.op, qa, qb, z);
        else { z[0] = qa[0].x; z[1] = qa[0].y; z[2] = qa[0].z; z[3] = qa[0].w; z[4] = qa[1].x; z[5] = qa[1].y; z[6] = qa[1].z; z[7] = qa[1].w; }
        *(float4*)(Zs + gr * PM_WZLD + gq) = make_float4(z[0], z[1], z[2], z[3]);
        *(float4*)(Zs + gr * PM_WZLD + gq + 4) = make_float4(z[4], z[5], z[6], z[7]);
#pragma unroll
        for (int v = 0; v < 8; ++v) *(float4*)(Ds + gr * PM_WLD + dq + 4 * v) = dv[v];
    };

    pm_f16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    if (r_beg < r_end) load(r_beg);
    for (int64_t r0 = r_beg; r0 < r_end; r0 += PM_WR) {                          // (r_beg, r_end and rows_pad are multiples of PM_WR)
        store();
        __syncthreads();
        if (r0 + PM_WR < r_end) load(r0 + PM_WR);
        if (active) {
#pragma unroll 4
            for (int kk = 0; kk < PM_WR; kk += 2) {
                float av[2], bv[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) av[i] = Zs[(kk + half) * PM_WZLD + i * 32 + l31];
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = Ds[(kk + half) * PM_WLD + cb + j * 32 + l31];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float* out = part + (int64_t)blockIdx.y * A.K * A.Hd;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t col = cb + j * 32 + l31;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int32_t m = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                if (m < lim && col < A.Hd) out[(int64_t)(kbase + m) * A.Hd + col] = acc[i][j][e];
            }
        }
}

// ---------------------------------------------------------------------------------------------------- reduce
// grad[e] (loss for the last e) = [first ? 0 : its value] + the sum, ascending, of the chunk's range partials (e < K Hd) or tile partials (b1, w2, b2, loss)
__global__ void __launch_bounds__(PM_THREADS) k_pmlp_reduce(int32_t K, int32_t Hd, int32_t HP, const float* __restrict__ part, int32_t ranges, const float* __restrict__ tp,
                                                            int32_t tiles, int32_t first, float* __restrict__ grad, float* __restrict__ loss) {
    const int64_t e = (int64_t)blockIdx.x * PM_THREADS + threadIdx.x, nw = (int64_t)K * Hd;
    if (e > nw + 2 * Hd + 1) return;
    float s;
    if (e < nw) {
        s = part[e];
        for (int32_t r = 1; r < ranges; ++r) s += part[(int64_t)r * nw + e];
    } else {
        const int32_t j = (int32_t)(e - nw);                                    // b1: db1 at HP + j;  w2: dw2 at j - Hd;  b2: 2 HP;  loss: 2 HP + 1
        const int32_t src = j < Hd ? HP + j : j < 2 * Hd ? j - Hd : 2 * HP + (j - 2 * Hd);
        const int64_t ts = 2 * HP + 4;
        s = tp[src];
        for (int32_t q = 1; q < tiles; ++q) s += tp[q * ts + src];
    }
    float* dst = e <= nw + 2 * Hd ? grad + e : loss;
    *dst = first ? s : *dst + s;
}

// ---------------------------------------------------------------------------------------------------- host
static int pm_check(const char* what, const gm_prop* p, const int32_t* d_pairs, int64_t n, int32_t op, const float* d_extra, int32_t S, const float* d_params, int32_t Hd) {
    GM_REQUIRE(p, GM_EINVAL, "%s: prop is NULL", what);
    GM_REQUIRE(Hd >= 1 && Hd <= PM_MAX_HD, GM_EINVAL, "%s: Hd = %d; 1 .. %d", what, Hd, PM_MAX_HD);
    GM_REQUIRE(S >= 0 && S <= PM_MAX_S, GM_EINVAL, "%s: S = %d; 0 .. %d", what, S, PM_MAX_S);
    GM_REQUIRE(op == GM_PROP_HADAMARD || op == GM_PROP_ABS_DIFF, GM_EINVAL, "%s: op = %d; GM_PROP_HADAMARD = 0, GM_PROP_ABS_DIFF = 1", what, op);
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_params && (d_extra || S == 0), GM_EINVAL, "%s: NULL argument (d_pairs %p, d_params %p, d_extra %p with S = %d)", what, (const void*)d_pairs,
               (const void*)d_params, (const void*)d_extra, S);
    return GM_OK;
}

static pm_args pm_make(const gm_prop* p, const int32_t* d_pairs, int64_t n, int32_t op, const float* d_extra, int32_t S, const float* d_params, int32_t Hd) {
    pm_args A;
    A.x = p->d; A.N = p->N; A.L1 = p->hops + 1; A.F = p->F; A.ld = p->ld;
    A.pairs = d_pairs; A.extra = d_extra; A.S = S; A.n = n;
    A.op = op; A.K = A.L1 * p->F + S; A.Hd = Hd; A.HP = (Hd + 63) / 64 * 64;
    A.W1 = d_params; A.b1 = d_params + (int64_t)A.K * Hd; A.w2 = A.b1 + Hd; A.b2 = A.w2 + Hd;
    return A;
}

extern "C" int32_t gm_prop_pair_mlp_tile(void) { return PM_T; }

extern "C" int32_t gm_prop_pair_mlp_dims(const gm_prop_t* p, int32_t S, int32_t Hd, int32_t* K, int64_t* n_params) {
    const char* what = "gm_prop_pair_mlp_dims";
    GM_REQUIRE(p, GM_EINVAL, "%s: prop is NULL", what);
    GM_REQUIRE(Hd >= 1 && Hd <= PM_MAX_HD, GM_EINVAL, "%s: Hd = %d; 1 .. %d", what, Hd, PM_MAX_HD);
    GM_REQUIRE(S >= 0 && S <= PM_MAX_S, GM_EINVAL, "%s: S = %d; 0 .. %d", what, S, PM_MAX_S);
    const int32_t k = (p->hops + 1) * p->F + S;
    if (K) *K = k;
    if (n_params) *n_params = (int64_t)k * Hd + 2 * Hd + 1;
    return GM_OK;
}

extern "C" int32_t gm_prop_pair_mlp_forward(const gm_prop_t* p, const int32_t* d_pairs, int64_t n, int32_t op, const float* d_extra, int32_t S, const float* d_params, int32_t Hd,
                                            float* d_logits, void* stream) {
    const char* what = "gm_prop_pair_mlp_forward";
    GM_TRY(pm_check(what, p, d_pairs, n, op, d_extra, S, d_params, Hd));
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_logits, GM_EINVAL, "%s: d_logits is NULL", what);
    const pm_args A = pm_make(p, d_pairs, n, op, d_extra, S, d_params, Hd);
    hipLaunchKernelGGL(k_pmlp_fwd<false>, dim3((unsigned)((n + PM_T - 1) / PM_T)), dim3(PM_THREADS), 0, (hipStream_t)stream, A, (const float*)nullptr, 0.f, d_logits, (float*)nullptr,
                       (float*)nullptr);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

extern "C" int32_t gm_prop_pair_mlp_step(const gm_prop_t* p, const int32_t* d_pairs, int64_t n, int32_t op, const float* d_extra, int32_t S, const float* d_labels,
                                         const float* d_params, int32_t Hd, float* d_logits, float* d_loss, float* d_grad, void* stream) {
    const char* what = "gm_prop_pair_mlp_step";
    GM_TRY(pm_check(what, p, d_pairs, n, op, d_extra, S, d_params, Hd));
    const int knob = gm_knob().pair_mlp_rows;
    GM_REQUIRE(knob >= 0, GM_EINVAL, "%s: pair_mlp_rows = %d", what, knob);
    GM_REQUIRE(d_loss && d_grad, GM_EINVAL, "%s: NULL argument (d_loss %p, d_grad %p)", what, (const void*)d_loss, (const void*)d_grad);
    const hipStream_t st = (hipStream_t)stream;
    const int32_t K = (p->hops + 1) * p->F + S;
    const int64_t n_params = (int64_t)K * Hd + 2 * Hd + 1;
    if (n == 0) {
        GM_HIP(hipMemsetAsync(d_grad, 0, (size_t)n_params * sizeof(float), st));
        GM_HIP(hipMemsetAsync(d_loss, 0, sizeof(float), st));
        return GM_OK;
    }
    GM_REQUIRE(d_labels, GM_EINVAL, "%s: d_labels is NULL", what);
    const int32_t HP = (Hd + 63) / 64 * 64;
    const int64_t R = std::min<int64_t>(knob ? knob : PM_ROWS, n);                                 // pairs per chunk
    const int64_t tiles_max = (R + PM_T - 1) / PM_T, rows_max = tiles_max * PM_T;
    // rows per weight-gradient range, ONE length for every chunk of the call (a multiple of PM_WR, at most PM_MAX_RANGES ranges in the largest chunk): a shorter last
    // chunk has fewer ranges of the same length, never more than `part` holds
    const int64_t rr = std::max<int64_t>(PM_RANGE, ((rows_max + PM_MAX_RANGES - 1) / PM_MAX_RANGES + PM_WR - 1) / PM_WR * PM_WR);
    const int64_t ranges_max = (rows_max + rr - 1) / rr;
    const int32_t ktiles = (p->hops + 1) * ((p->F + PM_WK - 1) / PM_WK) + (S + PM_WK - 1) / PM_WK;
    gm_scratch sc(st);
    float *dh = nullptr, *tp = nullptr, *part = nullptr;
    GM_TRY(sc.take(&dh, (size_t)(rows_max * HP)));
    GM_TRY(sc.take(&tp, (size_t)(tiles_max * (2 * HP + 4))));
    GM_TRY(sc.take(&part, (size_t)(ranges_max * K * Hd)));
    const float inv_n = 1.0f / (float)n;
    for (int64_t c0 = 0; c0 < n; c0 += R) {
        const int64_t nc = std::min<int64_t>(R, n - c0), tiles = (nc + PM_T - 1) / PM_T, rows_pad = tiles * PM_T, ranges = (rows_pad + rr - 1) / rr;
        GM_REQUIRE(tiles <= tiles_max && ranges <= ranges_max, GM_ERANGE, "%s: a chunk of %lld rows in %lld ranges passes the scratch of %lld rows in %lld ranges", what,
                   (long long)rows_pad, (long long)ranges, (long long)rows_max, (long long)ranges_max);
        const pm_args A = pm_make(p, d_pairs + 2 * c0, nc, op, S ? d_extra + c0 * S : nullptr, S, d_params, Hd);
        hipLaunchKernelGGL(k_pmlp_fwd<true>, dim3((unsigned)tiles), dim3(PM_THREADS), 0, st, A, d_labels + c0, inv_n, d_logits ? d_logits + c0 : (float*)nullptr, dh, tp);
        hipLaunchKernelGGL(k_pmlp_wgrad, dim3((unsigned)ktiles, (unsigned)ranges), dim3(PM_THREADS), 0, st, A, (const float*)dh, rr, rows_pad, part);
        hipLaunchKernelGGL(k_pmlp_reduce, dim3((unsigned)((n_params + 1 + PM_THREADS - 1) / PM_THREADS)), dim3(PM_THREADS), 0, st, K, Hd, HP, (const float*)part, (int32_t)ranges,
                           (const float*)tp, (int32_t)tiles, c0 == 0 ? 1 : 0, d_grad, d_loss);
        GM_HIP(hipGetLastError());
    }
    return GM_OK;
}
