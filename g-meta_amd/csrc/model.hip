// Classifier forward/backward (learner.py:134-175), prototypical losses (meta.py:14-79) and the
// first-order ProtoMAML inner/outer step (meta.py:101-173, 175-234) for ALL tasks of a meta-batch
// at once.  Each task (set) owns its fast weights; the K-loop runs here so that one FFI call is one
// meta-step and nothing returns to the host until the accuracies are read back.
#include <algorithm>
#include <atomic>
#include <map>
#include <stdlib.h>
#include "gm_internal.h"


// ================================================================================ small kernels
__device__ __forceinline__ float wave_sumf(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct HeadK {
    const float* H; int64_t ldh; int Hd;            // last GCN activation [rows, Hd]
    const int32_t* sub_off; const int32_t* centre; int nc; const int32_t* sub_set; const int32_t* set_sub_off;
    const float* params; int64_t pstride; int64_t wl_off, bl_off; int hc, C; int subs;
    int compact;                                    // 1: H holds only the centre rows, [subs*nc, Hd] in centre order (cone schedule)
    unsigned* dq_amax;                              // optional [sets * GM_BOUND_PAD] (zeroed): receives max |dQ| written for the set (gm_bound.h)
    int subs_per_set;                               // > 0: every set holds this many subgraphs (set t starts at t * subs_per_set: no load of set_sub_off ahead of everything else)
};

__device__ __forceinline__ int64_t centre_row(const HeadK& k, int s, int which) {
    return k.compact ? (int64_t)s * k.nc + which : (int64_t)k.sub_off[s] + k.centre[s * k.nc + which];
}

// Optional fused inner-loop SGD (meta.py:126,151): next_t[j] = cur_t[j] - lr * grad_t[j], written with the gradient.
struct SgdK { const float* cur; int64_t cur_stride; float* next; int64_t next_stride; float lr; };

// ---- address-space policies of the head kernels.  The fused kernel (k_head_loss) keeps a set's centre rows, head weights, logits and dlogits in LDS; the
// unfused kernels (k_head_fwd / k_proto / k_head_bwd: the public per-phase entry points) work on the global arrays.  Written with plain `float*` and a
// run-time `staged ? lds : global` choice, every access became a FLAT instruction (159 flat_load in the fused kernel: LDS data through the vector-memory
// path, several times an ds_read's latency, and both wait counters to drain) -- in a kernel that is one workgroup per task and nothing but latency.  The LDS
// pointers therefore carry their address space in the type, and the two variants are separate instantiations.
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(3))) int lds_int;
struct MemG { typedef float* F; typedef const float* CF; typedef const int32_t* CI; static constexpr bool lds = false; };
struct MemL { typedef lds_float* F; typedef const lds_float* CF; typedef const lds_int* CI; static constexpr bool lds = true; };
// Barrier between phases that exchange data through LDS only (MemL): lgkmcnt(0) + s_barrier.  __syncthreads() also drains the vector-memory counter, i.e.
// it waits for the acknowledgement of every global STORE issued before it (the prototypes, the loss / accuracy, the phase stamps: ~1 us each) -- results nobody in
// the block reads.  MemG exchanges the logits / dlogits through global memory and keeps the full barrier.
template <typename M> __device__ __forceinline__ void block_sync() {
    if constexpr (M::lds) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); else __syncthreads();
}

// logits[s,:] = F.linear(cat(h[c0], h[c1]), Wl, bl)  (learner.py:165-175); one wave per subgraph, a 16-lane group per output class: four classes
// are reduced at once with four shuffle steps (a wave-wide reduction per class was 6 dependent ds_bpermute round trips per logit).
// The association is the wave-wide version's, bit for bit: lane l of a group carries the partial sums of the former lanes l, l + 16, l + 32, l + 48
// (columns h = lane mod 64, ascending) and joins them the way the 32- and 16-lane butterfly steps did.  (Not pedantry: fixture g1_sampled_h2 holds rows
// whose layer-2 pre-activation is the bias alone, so the SIGN of a 1e-9-sized bias decides their relu' -- another rounding of the logits moved one
// meta-gradient entry of the flagged schedules by 150 % against the reference's golden value.)
// MemL: hs = the set's centre rows (subgraphs from s0, centre order: cat(h[c0], h[c1]) of a subgraph is contiguous), wl_s = [Wl | bl]; logits holds
// subgraphs [lbase, ..).  MemG: rows of k.H, the set's parameters.
template <typename M>
__device__ __forceinline__ void head_fwd_sub(const HeadK& k, int s, int lane, typename M::F logits, typename M::CF hs, int s0, typename M::CF wl_s, int lbase) {
    const int grp = lane >> 4, l = lane & 15;
    if constexpr (M::lds) {
        typename M::CF x = hs + (s - s0) * k.nc * k.Hd;
        for (int c0 = 0; c0 < k.C; c0 += 4) {
            const int c = c0 + grp, cc = min(c, k.C - 1);
            typename M::CF w = wl_s + cc * k.hc;
            float p[4] = {0.f, 0.f, 0.f, 0.f};
            if ((k.hc & 63) == 0) {                    // the reads of four 64-column steps (all of hc = 256) in flight together
#pragma unroll 4
                for (int hb = l; hb < k.hc; hb += 64) {
                    p[0] += x[hb] * w[hb]; p[1] += x[hb + 16] * w[hb + 16]; p[2] += x[hb + 32] * w[hb + 32]; p[3] += x[hb + 48] * w[hb + 48];
                }
            } else {
                for (int hb = l; hb < k.hc; hb += 64) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) { const int h = hb + 16 * m; if (h < k.hc) p[m] += x[h] * w[h]; }
                }
            }
            float acc = (p[0] + p[2]) + (p[1] + p[3]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (l == 0 && c < k.C) logits[(s - lbase) * k.C + c] = acc + wl_s[k.C * k.hc + c];
        }
    } else {
        const float* P = k.params + (int64_t)k.sub_set[s] * k.pstride;
        const float* h0 = k.H + centre_row(k, s, 0) * k.ldh;
        const float* h1 = k.nc == 2 ? k.H + centre_row(k, s, 1) * k.ldh : h0;
        for (int c0 = 0; c0 < k.C; c0 += 4) {
            const int c = c0 + grp, cc = min(c, k.C - 1);
            const float* w = P + k.wl_off + (int64_t)cc * k.hc;
            float p[4] = {0.f, 0.f, 0.f, 0.f};
            for (int hb = l; hb < k.hc; hb += 64) {
#pragma unroll
                for (int m = 0; m < 4; ++m) { const int h = hb + 16 * m; if (h < k.hc) p[m] += (h < k.Hd ? h0[h] : h1[h - k.Hd]) * w[h]; }
            }
            float acc = (p[0] + p[2]) + (p[1] + p[3]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (l == 0 && c < k.C) logits[(int64_t)(s - lbase) * k.C + c] = acc + P[k.bl_off + c];
        }
    }
}
__global__ __launch_bounds__(256) void k_head_fwd(HeadK k, float* logits) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s < k.subs) head_fwd_sub<MemG>(k, s, threadIdx.x & 63, logits, nullptr, 0, nullptr, 0);
}

// Backward of the head for one set per block: dWl, dbl into dparams; dQ_L (pre-zeroed) at the centre rows,
// already multiplied by relu'(H_L).  With Gc != NULL the rows go to a compact [subs*centres, Hd] matrix instead.
// dlogits holds subgraphs [dbase, ..).  MemL: hs / wl_s as above, crow_s = the rows of the set's centres; pre: u.cur of this thread's first Wl / bl entry was
// loaded by the caller.  s0 / s1: the set's subgraph range.  dbg: phase stamp 5 of block 0 (gm_head_loss_debug).
template <int NT, typename M>
__device__ __forceinline__ void head_bwd_set(const HeadK& k, int set, int tid, typename M::CF dlogits, float* dparams, int64_t dstride, float* dQ,
                                             float* Gc, const SgdK& u, typename M::CF hs, typename M::CF wl_s, int dbase, typename M::CI crow_s,
                                             bool pre, float pre_w, float pre_b, int s0, int s1, unsigned long long* dbg) {
    const float* P = k.params + (int64_t)set * k.pstride;
    auto wl = [&](int i) -> float { if constexpr (M::lds) return wl_s[i]; else return P[k.wl_off + i]; };                   // Wl[C, hc]
    auto feat = [&](int s, int which, int col) -> float {                                                                  // H_L at centre `which` of subgraph s
        if constexpr (M::lds) return hs[((s - s0) * k.nc + which) * k.Hd + col]; else return k.H[centre_row(k, s, which) * k.ldh + col];
    };
    auto crow = [&](int s, int which) -> int64_t { if constexpr (M::lds) return crow_s[(s - s0) * k.nc + which]; else return centre_row(k, s, which); };
    float* D = dparams + (int64_t)set * dstride;
    const int S = s1 - s0;
    for (int id = tid; id < k.C * k.hc; id += NT) {
        const int c = id / k.hc, h = id - c * k.hc;
        float acc = 0.f;
        if constexpr (M::lds) {     // column h of cat(h[c0], h[c1]) of subgraph s0 + j is hs[j * hc + h]: 32-bit index arithmetic, reads issued ahead
            typename M::CF hcol = hs + h;
            typename M::CF dcol = dlogits + (s0 - dbase) * k.C + c;
#pragma unroll 8
            for (int j = 0; j < S; ++j) acc += dcol[j * k.C] * hcol[j * k.hc];
        } else {
            for (int s = s0; s < s1; ++s) acc += dlogits[(int64_t)(s - dbase) * k.C + c] * (h < k.Hd ? feat(s, 0, h) : feat(s, 1, h - k.Hd));
        }
        D[k.wl_off + id] = acc;
        if (u.next) u.next[(int64_t)set * u.next_stride + k.wl_off + id] = ((pre && id == tid) ? pre_w : u.cur[(int64_t)set * u.cur_stride + k.wl_off + id]) - u.lr * acc;
    }
    for (int c = tid; c < k.C; c += NT) {
        float acc = 0.f;
#pragma unroll 8
        for (int s = s0; s < s1; ++s) acc += dlogits[(s - dbase) * k.C + c];
        D[k.bl_off + c] = acc;
        if (u.next) u.next[(int64_t)set * u.next_stride + k.bl_off + c] = ((pre && c == tid) ? pre_b : u.cur[(int64_t)set * u.cur_stride + k.bl_off + c]) - u.lr * acc;
    }
    if (dbg && set == 0 && tid == 0) dbg[5] = wall_clock64();
    // one thread per (subgraph, column); both centres of a pair stay in one thread (they may share a row).  dQ is all zeros when this runs and a row is the
    // centre of ONE subgraph, so the "+=" of learner.py's index_select backward is a plain store (no dependent read of dQ); the two centres of a pair may be
    // the same row: (0 + v0) + v1
    float dq_max = 0.f;
    constexpr int CMAX = 8;
    if (M::lds && !Gc && NT % k.Hd == 0 && k.C <= CMAX) {
        // dense dQ from the staged rows: a thread keeps ONE column (NT is a multiple of Hd) and walks the subgraphs NT / Hd apart -- no division in the loop,
        // the column's head weights in registers; per element the same operations in the same order as the general loop below
        const int col = tid % k.Hd, sstep = NT / k.Hd;
        float wv[2][CMAX];
#pragma unroll
        for (int which = 0; which < 2; ++which)
#pragma unroll
            for (int c = 0; c < CMAX; ++c) wv[which][c] = (which < k.nc && c < k.C) ? wl(c * k.hc + which * k.Hd + col) : 0.f;
        for (int j = tid / k.Hd; j < S; j += sstep) {
            typename M::CF dl_j = dlogits + (s0 - dbase + j) * k.C;
            float vv[2] = {0.f, 0.f};
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                if (which < k.nc) {
                    float v = 0.f;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) if (c < k.C) v += dl_j[c] * wv[which][c];
                    vv[which] = feat(s0 + j, which, col) > 0.f ? v : 0.f;
                }
            }
            const int64_t r0 = crow(s0 + j, 0);
            if (k.nc == 2) {
                const int64_t r1 = crow(s0 + j, 1);
                if (r1 == r0) vv[0] = vv[0] + vv[1]; else { dQ[r1 * k.ldh + col] = vv[1]; dq_max = fmaxf(dq_max, fabsf(vv[1])); }
            }
            dQ[r0 * k.ldh + col] = vv[0];
            dq_max = fmaxf(dq_max, fabsf(vv[0]));
        }
    } else {
        for (int id = tid; id < S * k.Hd; id += NT) {
            const int s = s0 + id / k.Hd, col = id % k.Hd;
            float vv[2] = {0.f, 0.f};
            for (int which = 0; which < k.nc; ++which) {
                float v = 0.f;
                for (int c = 0; c < k.C; ++c) v += dlogits[(s - dbase) * k.C + c] * wl(c * k.hc + which * k.Hd + col);
                const float hval = feat(s, which, col);
                if (Gc) Gc[((int64_t)s * k.nc + which) * k.Hd + col] = hval > 0.f ? v : 0.f;     // compact rows (sparse backward / cone)
                else vv[which] = hval > 0.f ? v : 0.f;
            }
            if (!Gc) {
                const int64_t r0 = crow(s, 0);
                if (k.nc == 2) {
                    const int64_t r1 = crow(s, 1);
                    if (r1 == r0) vv[0] = vv[0] + vv[1]; else { dQ[r1 * k.ldh + col] = vv[1]; dq_max = fmaxf(dq_max, fabsf(vv[1])); }
                }
                dQ[r0 * k.ldh + col] = vv[0];
                dq_max = fmaxf(dq_max, fabsf(vv[0]));
            }
        }
    }
    if (k.dq_amax && !Gc) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) dq_max = fmaxf(dq_max, __shfl_xor(dq_max, o));
        if ((tid & 63) == 0 && dq_max > 0.f) atomicMax(k.dq_amax + (int64_t)set * GM_BOUND_PAD, __float_as_uint(dq_max));      // (a handful per set)
    }
}
__global__ __launch_bounds__(256) void k_head_bwd(HeadK k, const float* dlogits, float* dparams, int64_t dstride, float* dQ, float* Gc) {
    const int set = blockIdx.x;
    head_bwd_set<256, MemG>(k, set, threadIdx.x, dlogits, dparams, dstride, dQ, Gc, SgdK{nullptr, 0, nullptr, 0, 0.f}, nullptr, nullptr, 0, nullptr, false, 0.f, 0.f,
                            k.set_sub_off[set], k.set_sub_off[set + 1], nullptr);
}

// Prototypical loss for one set per block (meta.py:28-79).  rows: [sets, Ct, n] global subgraph ids grouped by
// sorted class.  mode 0 = support (prototypes = class means of the same rows), 1 = query (prototypes given).
struct ProtoK {
    const float* logits; int D; const int32_t* rows; int Ct, n; int mode;      // Ct, n: the LARGEST class count / rows per class over the sets
    const float* protos_in; float* protos_out; float* loss; float* acc; int64_t ld_out; int col_out;
    float* dlogits; float* dprotos;
    int row_base;                         // logits / dlogits hold subgraphs [row_base, ...): 0 for the global arrays, the set's first
                                          // subgraph when the fused kernel keeps them in LDS
    const int32_t* tab;                   // [sets*3] per set: offset into rows, classes, rows per class (every task keeps its own class
                                          // layout, like the per-task proto_loss calls of meta.py:118-157); prototypes are strided by Ct
    int uniform;                          // every set has Ct classes of n rows at offset set * Ct * n (the usual case): the kernels take the layout from the arguments
};                                        // instead of a dependent load of `tab` ahead of the class rows
// Ragged-task mode only: a launch may hold sets whose classes have unequal row counts (the kernels' RGK instantiations).  Such a set t has tab[3t + 2] =
// -(its scored rows) and its block of `rows` is [class starts (Ct_t + 1, relative to the class rows) | class rows]; balanced sets of the same launch keep the
// [off, Ct, n] form and the balanced code.  ProtoK::n of such a launch is rounded up so that Ct * n also covers the scored rows of every ragged set (LDS carve).

template <typename XP>
__device__ __forceinline__ float sqdist(XP x, const lds_float* p, int D) {
    float d = 0.f;
    for (int k = 0; k < D; ++k) { const float t = x[k] - p[k]; d += t * t; }
    return d;
}

// LDS of a set: prototypes [Ct*D] | lse [Ct*n] | block-sum scratch [2*NT] | A [Ct*n*Ct] (only when it is at most PROTO_A_MAX floats).
// A holds -dist(q, c) and then G[q,c] = (softmax(-d)[q,c] - [c == class(q)]) / Q: every later phase reads it instead of redoing the distance and the
// exponential, and the loops that must stay serial (a class sum over its rows, a prototype's gradient over the queries: their order is part of the
// result) carry nothing but LDS reads that can be issued ahead.  The kernel is one workgroup per task and pure latency.
// logits / dlogits / rows: the arrays the set is scored on -- k's global ones (MemG; rows already offset to the set) or the fused kernel's LDS copies (MemL).
#define PROTO_A_MAX 8192
// class of scored row q of a ragged set: the last class that starts at or before q (a class without rows -- a query set may have some -- starts where the
// next one does, and is never the answer)
template <typename CI>
__device__ __forceinline__ int ragged_class(CI coff, int Ct, int q) {
    int lo = 0, hi = Ct - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (coff[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// RG: the set is ragged (see ProtoK): `rows` is its block [class starts | class rows], a row's class and a class's row count come from the class starts
// (in LDS when the caller staged the block).  The LDS carve, the arithmetic and the summation orders are the balanced variant's.
template <int NT, typename M, bool RG = false>
__device__ __forceinline__ void proto_set(const ProtoK& k, int set, int tid, lds_float* sm, typename M::CF logits, typename M::F dlogits, typename M::CI rows,
                                          bool have_proto = false, float proto_pre = 0.f) {      // have_proto: protos_in[set][tid] was loaded by the caller (tid < Ct * D)
    const int Ct = (k.uniform && !RG) ? k.Ct : k.tab[set * 3 + 1], n = RG ? 0 : (k.uniform ? k.n : k.tab[set * 3 + 2]);
    const int Q = RG ? -k.tab[set * 3 + 2] : Ct * n, D = k.D, rb = k.row_base;
    typename M::CI coff = rows;         // RG: class c scores rows[coff[c] .. coff[c + 1])
    if constexpr (RG) rows += Ct + 1;
    auto cls = [&](int q) -> int { if constexpr (RG) return ragged_class(coff, Ct, q); else return q / n; };
    auto own = [&](int q, int c) -> bool { if constexpr (RG) return q >= coff[c] && q < coff[c + 1]; else return c == q / n; };
    lds_float* protos = sm;             // [Ct*D]   (LDS sized for the largest set)
    lds_float* lse = sm + k.Ct * D;     // [Q]
    lds_float* red = lse + k.Ct * k.n;  // [2 * NT]
    lds_float* A = red + 2 * NT;        // [Q * Ct]
    const bool useA = (int64_t)k.Ct * k.n * k.Ct <= PROTO_A_MAX;
    for (int id = tid; id < Ct * D; id += NT) {
        const int c = id / D, d = id - c * D;
        float p;
        if (k.mode == 0) {
            p = 0.f;
            if constexpr (RG) {
                const int r0 = coff[c], r1 = coff[c + 1];
#pragma unroll 4
                for (int r = r0; r < r1; ++r) p += logits[(rows[r] - rb) * D + d];
                p /= (float)(r1 - r0);
            } else {
#pragma unroll 4
                for (int r = 0; r < n; ++r) p += logits[(rows[c * n + r] - rb) * D + d];
                p /= (float)n;                                                      // .mean(0) (meta.py:41)
            }
            if (k.protos_out) k.protos_out[(int64_t)set * k.Ct * D + id] = p;
        } else {
            p = (have_proto && id == tid) ? proto_pre : k.protos_in[(int64_t)set * k.Ct * D + id];
        }
        protos[id] = p;
    }
    block_sync<M>();
    if (useA) {
        for (int id = tid; id < Q * Ct; id += NT) {
            const int q = id / Ct, c = id - q * Ct;
            A[id] = -sqdist(logits + (rows[q] - rb) * D, protos + c * D, D);      // -dists (meta.py:44-45)
        }
        block_sync<M>();
    }
    float lpart = 0.f, apart = 0.f;
    for (int q = tid; q < Q; q += NT) {
        typename M::CF x = logits + (rows[q] - rb) * D;
        const int tgt = cls(q);
        float m = -INFINITY, at = 0.f;
        for (int c = 0; c < Ct; ++c) {
            const float a = useA ? A[q * Ct + c] : -sqdist(x, protos + c * D, D);
            m = fmaxf(m, a);
            if (c == tgt) at = a;
        }
        float se = 0.f;
        for (int c = 0; c < Ct; ++c) se += expf((useA ? A[q * Ct + c] : -sqdist(x, protos + c * D, D)) - m);
        const float lg = logf(se);
        lse[q] = m + lg;
        lpart += -((at - m) - lg);                                                   // -log_p[q, class(q)], log_softmax = (x - max) - log(sum exp(x - max))
        // y_hat = log_p_y.max(2) (meta.py:52,76): the prediction is the FIRST maximum of the fp32 LOG-PROBABILITIES, not of the distances --
        // when the logits are tiny (distances below one ulp of log(sum)) every class rounds to the same log-probability and the reference
        // predicts class 0; reproduced (fixture g8_wide_scales)
        float bl = -INFINITY; int best = 0;
        for (int c = 0; c < Ct; ++c) {
            const float lp = ((useA ? A[q * Ct + c] : -sqdist(x, protos + c * D, D)) - m) - lg;
            if (lp > bl) { bl = lp; best = c; }
        }
        apart += (best == tgt) ? 1.f : 0.f;
    }
    // block sum of (loss, correct): wave shuffles, then the first wave adds the NT / 64 wave partials (two barriers instead of log2 NT)
    lpart = wave_sumf(lpart); apart = wave_sumf(apart);
    if ((tid & 63) == 0) { red[tid >> 6] = lpart; red[NT + (tid >> 6)] = apart; }
    block_sync<M>();
    if (tid < 64) {
        float l2 = tid < NT / 64 ? red[tid] : 0.f, a2 = tid < NT / 64 ? red[NT + tid] : 0.f;
        l2 = wave_sumf(l2); a2 = wave_sumf(a2);
        if (tid == 0) {
            k.loss[(int64_t)set * k.ld_out + k.col_out] = l2 / (float)Q;
            k.acc[(int64_t)set * k.ld_out + k.col_out] = a2 / (float)Q;
        }
    }
    if (!dlogits) return;
    // G[q,c] = (softmax(-d)[q,c] - [c == tgt(q)]) / Q ;  d(-d_qc)/dx_q = -2 (x_q - p_c) ; d(-d_qc)/dp_c = +2 (x_q - p_c)
    const float invQ = 1.f / (float)Q;
    if (useA) {
        for (int id = tid; id < Q * Ct; id += NT) {
            const int q = id / Ct, c = id - q * Ct;
            A[id] = (expf(A[id] - lse[q]) - (own(q, c) ? 1.f : 0.f)) * invQ;
        }
        block_sync<M>();
    }
    for (int id = tid; id < Q * D; id += NT) {
        const int q = id / D, d = id - q * D;
        typename M::CF x = logits + (rows[q] - rb) * D;
        const int tgt = (RG && useA) ? 0 : cls(q);      // (only the branch without the A table needs it)
        float s = 0.f;
        for (int c = 0; c < Ct; ++c) {
            const float g = useA ? A[q * Ct + c] : (expf(-sqdist(x, protos + c * D, D) - lse[q]) - (c == tgt ? 1.f : 0.f)) * invQ;
            s += g * -2.f * (x[d] - protos[c * D + d]);
        }
        dlogits[(rows[q] - rb) * D + d] = s;
    }
    block_sync<M>();
    for (int id = tid; id < Ct * D; id += NT) {
        const int c = id / D, d = id - c * D;
        const float pd = protos[id];
        float s = 0.f;
        if (useA) {
#pragma unroll 8
            for (int q = 0; q < Q; ++q) s += A[q * Ct + c] * 2.f * (logits[(rows[q] - rb) * D + d] - pd);
        } else {
            for (int q = 0; q < Q; ++q) {
                typename M::CF x = logits + (rows[q] - rb) * D;
                const float g = (expf(-sqdist(x, protos + c * D, D) - lse[q]) - (own(q, c) ? 1.f : 0.f)) * invQ;
                s += g * 2.f * (x[d] - pd);
            }
        }
        if (k.mode == 0) {
            if constexpr (RG) {
                const int r0 = coff[c], r1 = coff[c + 1];
#pragma unroll 4
                for (int r = r0; r < r1; ++r) dlogits[(rows[r] - rb) * D + d] += s / (float)(r1 - r0);
            } else {
#pragma unroll 4
                for (int r = 0; r < n; ++r) dlogits[(rows[c * n + r] - rb) * D + d] += s / (float)n;
            }
        } else if (k.dprotos) {
            k.dprotos[(int64_t)set * k.Ct * D + id] = s;
        }
    }
}

template <bool RGK>      // RGK: the launch holds ragged sets (see ProtoK)
__global__ __launch_bounds__(256) void k_proto(ProtoK k) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int set = blockIdx.x;
    if constexpr (RGK) {
        if (k.tab[set * 3 + 2] < 0) { proto_set<256, MemG, true>(k, set, threadIdx.x, (lds_float*)sm, k.logits, k.dlogits, k.rows + k.tab[set * 3]); return; }
    }
    proto_set<256, MemG>(k, set, threadIdx.x, (lds_float*)sm, k.logits, k.dlogits, k.rows + (k.uniform ? set * k.Ct * k.n : k.tab[set * 3]));
}

// Head forward + prototypical loss (+ head backward and the SGD of the head's own parameters) of one set per block: the
// five launches between the last GCN layer of a forward and the first weight gradient of its backward, in one.
#define HL_THREADS 1024     // largest workgroup of k_head_loss (LDS sizing)
// RGK: the launch holds ragged sets (ragged-task mode, see ProtoK): a kernel of its own, so that the kernel every other launch runs is the one it always ran
// (with both variants in one kernel the balanced path measured 0.9 us per launch slower at the FirstMM shape)
template <int NT, bool RGK = false>
__global__ __launch_bounds__(NT) void k_head_loss(HeadK hk, float* logits, ProtoK pk, int do_bwd, float* dparams, int64_t dstride, float* dQ,
                                                          float* Gc, SgdK u, int stage, int proto_floats, int copy_out, unsigned long long* dbg) {
    extern __shared__ __attribute__((aligned(16))) float sm_generic[];
    lds_float* sm = (lds_float*)sm_generic;
    const int set = blockIdx.x, tid = threadIdx.x;
#define HL_STAMP(K) do { if (dbg && set == 0 && tid == 0) dbg[K] = wall_clock64(); } while (0)      // phase timeline of block 0 (tools/head_loss_probe.py)
    HL_STAMP(0);
    const long long cyc0 = dbg ? clock64() : 0;      // shader-clock cycles next to the constant-clock stamps: stamp 7 = cycles spent (what clock the probe ran at)
    const int s0 = hk.subs_per_set ? set * hk.subs_per_set : hk.set_sub_off[set], s1 = hk.subs_per_set ? s0 + hk.subs_per_set : hk.set_sub_off[set + 1], S = s1 - s0, D = pk.D;
    // the head's own SGD inputs (w - lr * g, meta.py:126,151) go out with the first round trip instead of behind the loss
    const bool pre = do_bwd && u.next != nullptr;
    float pre_w = 0.f, pre_b = 0.f;
    if (pre) {
        if (tid < hk.C * hk.hc) pre_w = u.cur[(int64_t)set * u.cur_stride + hk.wl_off + tid];
        if (tid < hk.C) pre_b = u.cur[(int64_t)set * u.cur_stride + hk.bl_off + tid];
    }
    // ... and so do the prototypes a query loss is scored against (mode 1; uniform class layout: the set's are at set * Ct * D)
    const bool ragged = RGK && pk.tab[set * 3 + 2] < 0;
    const bool have_proto = stage && pk.mode == 1 && pk.uniform && pk.Ct * D <= NT;
    float proto_pre = 0.f;
    if (have_proto && tid < pk.Ct * D) proto_pre = pk.protos_in[(int64_t)set * pk.Ct * D + tid];
    if (!stage) {
        // everything in the global arrays (sets too large for LDS): the three phases with L2 round trips in between
        if (pk.dlogits) for (int id = tid; id < S * D; id += NT) pk.dlogits[(int64_t)s0 * D + id] = 0.f;   // rows outside the class tables
        for (int s = s0 + (tid >> 6); s < s1; s += NT / 64) head_fwd_sub<MemG>(hk, s, tid & 63, logits, nullptr, 0, nullptr, 0);
        __syncthreads();          // workgroup-scope fence: the logits / zeros written above are visible to the whole block
        HL_STAMP(3);
        if constexpr (RGK) { if (ragged) proto_set<NT, MemG, true>(pk, set, tid, sm, logits, pk.dlogits, pk.rows + pk.tab[set * 3]); }
        if (!ragged) proto_set<NT, MemG>(pk, set, tid, sm, logits, pk.dlogits, pk.rows + (pk.uniform ? set * pk.Ct * pk.n : pk.tab[set * 3]));
        HL_STAMP(4);
        if (!do_bwd) return;
        __syncthreads();
        head_bwd_set<NT, MemG>(hk, set, tid, pk.dlogits, dparams, dstride, dQ, Gc, u, nullptr, nullptr, 0, nullptr, pre, pre_w, pre_b, s0, s1, dbg);
        HL_STAMP(6);
        return;
    }
    // staged: everything the three phases share stays in LDS -- the set's centre rows of H_L, its head weights, its
    // logits and dlogits -- so that a phase costs LDS latency instead of an L2 round trip (the kernel is pure latency)
    lds_float* hs = sm + proto_floats;                                      // [S * nc, Hd] centre rows of H_L, centre order
    lds_float* wl_s = hs + S * hk.nc * hk.Hd;                               // [C * hc | C]  Wl | bl
    lds_float* lg_s = wl_s + hk.C * hk.hc + hk.C;                           // [S, D] logits
    lds_float* dl_s = lg_s + S * D;                                         // [S, D] dlogits
    lds_int* crow = (lds_int*)(dl_s + S * D);                               // [S * nc] row of every centre
    lds_int* rows_l = crow + S * hk.nc;                                     // [Ct * n] the set's class rows (subgraph ids); ragged set: [class starts | class rows]
    const float* P = hk.params + (int64_t)set * hk.pstride;
    const int nq = S * hk.nc;
    // first round trip, everything that needs no other load: centre rows (two dependent loads each), class rows, head weights
    for (int q = tid; q < nq; q += NT) crow[q] = (int)centre_row(hk, s0 + q / hk.nc, q % hk.nc);
    {
        const int off = pk.uniform ? set * pk.Ct * pk.n : pk.tab[set * 3];
        const int Qs = pk.uniform ? pk.Ct * pk.n : (ragged ? pk.tab[set * 3 + 1] + 1 - pk.tab[set * 3 + 2] : pk.tab[set * 3 + 1] * pk.tab[set * 3 + 2]);
        for (int q = tid; q < Qs; q += NT) rows_l[q] = pk.rows[off + q];
    }
    for (int id = tid; id < hk.C * hk.hc; id += NT) wl_s[id] = P[hk.wl_off + id];
    for (int id = tid; id < hk.C; id += NT) wl_s[hk.C * hk.hc + id] = P[hk.bl_off + id];
    block_sync<MemL>();
    HL_STAMP(1);
    // second round trip: the centre rows of H_L, all loads of a thread in flight together (16-byte loads when the rows allow it).  (The first version was a
    // serial chain of 18 dependent global loads per thread.)
    if ((hk.Hd & 3) == 0 && (hk.ldh & 3) == 0 && ((uintptr_t)hk.H & 15) == 0) {
        const int hd4 = hk.Hd >> 2, total4 = nq * hd4;
        typedef float f4v __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) f4v lds_f4v;
        for (int id0 = tid; id0 < total4; id0 += 8 * NT) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int id = min(id0 + j * NT, total4 - 1), q = id / hd4, c4 = id - q * hd4;
                v[j] = *reinterpret_cast<const float4*>(hk.H + (int64_t)crow[q] * hk.ldh + c4 * 4);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int id = id0 + j * NT; if (id < total4) { const f4v t = {v[j].x, v[j].y, v[j].z, v[j].w}; *(lds_f4v*)(hs + id * 4) = t; } }
        }
    } else {
        const int total = nq * hk.Hd;
        for (int id0 = tid; id0 < total; id0 += 8 * NT) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int id = min(id0 + j * NT, total - 1), q = id / hk.Hd, col = id - q * hk.Hd;
                v[j] = hk.H[(int64_t)crow[q] * hk.ldh + col];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { const int id = id0 + j * NT; if (id < total) hs[id] = v[j]; }
        }
    }
    lds_float* dl = pk.dlogits ? dl_s : nullptr;        // (pk.dlogits only says WHETHER the gradient is wanted; the global array is written with copy_out)
    if (dl) for (int id = tid; id < S * D; id += NT) dl_s[id] = 0.f;
    block_sync<MemL>();
    HL_STAMP(2);
    if (dbg && set == 0 && (tid & 63) == 0) dbg[8 + (tid >> 6)] = wall_clock64();
    for (int s = s0 + (tid >> 6); s < s1; s += NT / 64) head_fwd_sub<MemL>(hk, s, tid & 63, lg_s, hs, s0, wl_s, s0);
    if (dbg && set == 0 && (tid & 63) == 0) dbg[24 + (tid >> 6)] = wall_clock64();      // per-wave start / end of the logits phase
    block_sync<MemL>();
    HL_STAMP(3);
    ProtoK pl = pk;
    pl.row_base = s0;                                   // the LDS copies hold the set's subgraphs only
    if constexpr (RGK) { if (ragged) proto_set<NT, MemL, true>(pl, set, tid, sm, lg_s, dl, rows_l); }
    if (!ragged) proto_set<NT, MemL>(pl, set, tid, sm, lg_s, dl, rows_l, have_proto, proto_pre);
    HL_STAMP(4);
    if (copy_out) {  // the global copies (the public gm_proto_loss_* shape; nobody inside gm_meta_step reads them): logits always, dlogits when requested
        block_sync<MemL>();
        for (int id = tid; id < S * D; id += NT) {
            logits[(int64_t)s0 * D + id] = lg_s[id];
            if (dl) pk.dlogits[(int64_t)s0 * D + id] = dl_s[id];
        }
    }
    if (!do_bwd) return;
    block_sync<MemL>();
    head_bwd_set<NT, MemL>(hk, set, tid, dl_s, dparams, dstride, dQ, Gc, u, hs, wl_s, s0, crow, pre, pre_w, pre_b, s0, s1, dbg);
    HL_STAMP(6);
    if (dbg && set == 0 && tid == 0) dbg[7] = (unsigned long long)(clock64() - cyc0);
#undef HL_STAMP
}

// Prototype path back into the support logits (prototype_c = mean of the class's first n rows).
__global__ void k_protos_to_dlogits(const float* dprotos, const int32_t* rows, const int32_t* tab, int CtMax, int D, float* dlogits) {
    const int set = blockIdx.x, Ct = tab[set * 3 + 1], n = tab[set * 3 + 2];
    rows += tab[set * 3];
    for (int id = threadIdx.x; id < Ct * n * D; id += blockDim.x) {
        const int q = id / D, d = id - q * D, c = q / n;
        dlogits[(int64_t)rows[q] * D + d] = dprotos[((int64_t)set * CtMax + c) * D + d] / (float)n;
    }
}

// Scoring of query subgraphs against their set's prototypes (gm_proto_predict): one wave per subgraph, as k_head_fwd, so a set may hold any number of
// subgraphs.  Per subgraph the same operations in the same order as k_head_loss's: the head of head_fwd_sub, a_c = -sqdist to every prototype, then
// proto_set's log-softmax (a - m) - log(sum_c exp(a_c - m)) in class order and its FIRST maximum (class 0 when every entry is NaN or all round equal).
// LDS per wave: the set's prototypes [c_task, D] and a_c [c_task].  logits: [subs, D] (written, then read back by the same block); logp: [subs, c_task],
// -inf at and above the set's class count; pred: [subs].
__global__ __launch_bounds__(256) void k_head_predict(HeadK k, const float* protos, int c_task, const int32_t* n_cls, float* logits, float* logp, int32_t* pred) {
    extern __shared__ __attribute__((aligned(16))) float sm_generic[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, s = blockIdx.x * 4 + w, D = k.C;
    lds_float* pw = (lds_float*)sm_generic + w * c_task * (D + 1);
    lds_float* aw = pw + c_task * D;
    const bool live = s < k.subs;
    const int set = live ? k.sub_set[s] : 0;
    const int nt = live ? n_cls[set] : 0;
    if (live) {
        for (int id = lane; id < nt * D; id += 64) pw[id] = protos[(int64_t)set * c_task * D + id];
        head_fwd_sub<MemG>(k, s, lane, logits, nullptr, 0, nullptr, 0);
    }
    __syncthreads();          // workgroup-scope fence: the logits written above are visible to the whole block, as in k_head_loss
    const float* x = logits + (int64_t)s * D;
    for (int c = lane; c < nt; c += 64) aw[c] = -sqdist(x, pw + c * D, D);
    __syncthreads();
    if (!live) return;
    float m = -INFINITY;
    for (int c = 0; c < nt; ++c) m = fmaxf(m, aw[c]);
    float se = 0.f;
    for (int c = 0; c < nt; ++c) se += expf(aw[c] - m);
    const float lg = logf(se);
    float* lp = logp + (int64_t)s * c_task;
    for (int c = lane; c < c_task; c += 64) lp[c] = c < nt ? (aw[c] - m) - lg : -INFINITY;
    if (lane == 0) {
        float bl = -INFINITY; int best = 0;
        for (int c = 0; c < nt; ++c) { const float v = (aw[c] - m) - lg; if (v > bl) { bl = v; best = c; } }
        pred[s] = best;
    }
}

// gm_meta_adapt's outputs in the caller's layouts: fw_out[t] = fw[t] without the `shift` zero rows at `cut` (k_finalize's unpadding), and the
// prototypes [T, Ct, D] (set t's first tab[3t + 1] classes) restrided to [T, c_task, D] with zero rows at and above the set's class count
__global__ void k_adapt_out(const float* fw, int64_t fw_in_stride, int64_t P, int64_t cut, int64_t shift, float* fw_out, int64_t fw_stride,
                            const float* protos, int Ct, const int32_t* tab, int c_task, int D, float* protos_out) {
    const int t = blockIdx.y;
    const int64_t step = (int64_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    for (int64_t i = i0; i < P; i += step) fw_out[t * fw_stride + i] = fw[t * fw_in_stride + (i < cut ? i : i + shift)];
    const int nt = tab[t * 3 + 1];
    for (int64_t id = i0; id < (int64_t)c_task * D; id += step)
        protos_out[(int64_t)t * c_task * D + id] = id < (int64_t)nt * D ? protos[(int64_t)t * Ct * D + id] : 0.f;
}

// k_pad_params for one parameter vector per set: out[t] (stride ostride) = src[t] (stride sstride) with `shift` zeros inserted at `cut`
__global__ void k_pad_params_sets(const float* src, int64_t sstride, int64_t P, int64_t cut, int64_t shift, float* out, int64_t ostride) {
    const int t = blockIdx.y;
    for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < P + shift; id += (int64_t)gridDim.x * blockDim.x)
        out[t * ostride + id] = id < cut ? src[t * sstride + id] : (id < cut + shift ? 0.f : src[t * sstride + id - shift]);
}

// Row-sparse backward, expansion through the transposed aggregate: for every in-edge e = (u -> centre k)
//   G1[e,:] = norm[u] * relu'(H1[u,:]) * T2[k,:]      (dQ_{L-1} restricted to the rows that can be non-zero)
__global__ void k_expand_edges(const float* T2, const float* H1, int F, const int32_t* e_row, const int32_t* e_par, const float* e_norm,
                               int n_e, float* G1) {
    const int64_t tot = (int64_t)n_e * F;
    for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < tot; id += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(id / F), f = (int)(id - (int64_t)e * F);
        const float h = H1[(int64_t)e_row[e] * F + f];
        G1[id] = h > 0.f ? e_norm[e] * T2[(int64_t)e_par[e] * F + f] : 0.f;
    }
}

// WT[t][k][n] = W_t[n][k]: the dZ GEMM (dQ @ W^T) then runs as a plain row-major product on the DMA-fed kernel.
// W_t = params + t*pstride + w_off, [fi, fo] row-major; WT_t [fo, fi].  32x32 tiles through LDS, grid (fo/32, fi/32, sets).
__global__ __launch_bounds__(256) void k_transpose_w(const float* params, int64_t pstride, int64_t w_off, int fi, int fo, float* WT) {
    __shared__ float tile[32][33];
    const int t = blockIdx.z, k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const float* W = params + (int64_t)t * pstride + w_off;
    float* O = WT + (int64_t)t * fi * fo;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) { const int n = n0 + r, k = k0 + tx; tile[r][tx] = (n < fi && k < fo) ? W[(int64_t)n * fo + k] : 0.f; }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) { const int k = k0 + r, n = n0 + tx; if (k < fo && n < fi) O[(int64_t)k * fi + n] = tile[tx][r]; }
}

// db[set, n] = sum over the set's rows [set_off[set], set_off[set+1]) of G[row, n]   (cone schedule, multiply-first layers)
__global__ void k_colsum_rows(const float* G, int64_t ldg, int N, const int32_t* set_off, float* db, int64_t db_stride, SgdK u, int64_t b_off) {
    const int set = blockIdx.x, r0 = set_off[set], r1 = set_off[set + 1];
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float s = 0.f;
        for (int r = r0; r < r1; ++r) s += G[(int64_t)r * ldg + n];
        db[(int64_t)set * db_stride + n] = s;
        if (u.next) u.next[(int64_t)set * u.next_stride + b_off + n] = u.cur[(int64_t)set * u.cur_stride + b_off + n] - u.lr * s;
    }
}

// out = [ sum_t (gq+gp) | sum_t lq[t,:] | sum_t aq[t,:] | T | aq[t,:] ... ]
// (cut, shift): the kernels' parameter layout has `shift` extra floats after position `cut` (zero-padded W_1 rows when the store pads
// its feature columns); `out` uses the caller's layout.
// The last float is the step's violation word (gm_bound.h GM_VIOL_*; 0 unless the opt-in two-piece kernels found one of their bounds broken).  A step
// with a violation also reports losses_q[K] = NaN, so that every rank of a sharded meta-batch skips the optimiser step on the REDUCED loss
// (meta.py:163) and the host mirror can re-run the step with the three-piece kernels.
__global__ void k_finalize(const float* gq, const float* gp, int64_t stride, int64_t P, int T, const float* lq, const float* aq, int K1, float* out,
                           int64_t cut, int64_t shift, const unsigned* viol) {
    const int64_t tot = P + 2 * K1 + 1 + (int64_t)T * K1;
    const unsigned vw = viol ? *viol : 0u;
    for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id <= tot; id += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (id == tot) { out[id] = (float)vw; continue; }
        if (id < P) { const int64_t src = id < cut ? id : id + shift; if (gq) for (int t = 0; t < T; ++t) s += gq[t * stride + src] + gp[t * stride + src]; }
        else if (id < P + K1) { for (int t = 0; t < T; ++t) s += lq[t * K1 + (id - P)]; if (vw && id == P + K1 - 1) s = __uint_as_float(0x7fc00000u); }
        else if (id < P + 2 * K1) { for (int t = 0; t < T; ++t) s += aq[t * K1 + (id - P - K1)]; }
        else if (id == P + 2 * K1) s = (float)T;
        else s = aq[id - P - 2 * K1 - 1];
        out[id] = s;
    }
}

// ================================================================================ workspace carving
struct Carver {
    char* base; int64_t used = 0, cap;
    Carver(void* p, int64_t c) : base((char*)p), cap(c) {}
    template <class T> T* take(int64_t n) {
        const int64_t bytes = ((n > 0 ? n : 1) * (int64_t)sizeof(T) + 255) / 256 * 256;
        T* r = base ? (T*)(base + used) : nullptr;
        used += bytes;
        return r;
    }
    bool ok() const { return !base || used <= cap; }
};

// Split-bf16 operand planes of the fast weights fw_1..fw_K, written by the weight-gradient reduction that produces each vector
// (gm_wgrad_args::pl_fwd / pl_dz) and looked up by the GEMMs that consume it -- on either stream; the vector's own ready event
// orders them.  One slot per (k, layer, orientation); theta (shared by all tasks) is split on the fly: one set, one tiny launch.
#define GM_W_HEADROOM 1024.f
struct PlaneDir {
    const float* fw0 = nullptr; int64_t TP = 0; int K = 0;                  // fw_k = fw0 + (k-1) * TP, k = 1..K
    uint16_t* base = nullptr; int64_t per_k = 0;                            // planes of fw_k at base + (k-1) * per_k
    int64_t off[GM_MAX_GCN][2] = {};                                        // [layer][0 fwd, 1 dz] inside a k block; -1 = not kept
    bool valid[64][GM_MAX_GCN][2] = {};
    int index_of(const float* params) const {                               // 1..K, or 0
        if (!base || !fw0 || params < fw0) return 0;
        const int64_t d = params - fw0;
        if (d % TP) return 0;
        const int64_t k = d / TP + 1;
        return (k >= 1 && k <= K && k < 64) ? (int)k : 0;
    }
    uint16_t* slot(int k, int l, int o) const { return (k && off[l][o] >= 0) ? base + (int64_t)(k - 1) * per_k + off[l][o] : nullptr; }
    uint16_t* lookup(const float* params, int l, int o) const { const int k = index_of(params); return (k && off[l][o] >= 0 && valid[k][l][o]) ? slot(k, l, o) : nullptr; }
    // Weight bound for the two-piece fp16 planes (gm_bound.h): wam[l * GM_BOUND_PAD] = bit pattern of max |W_l| of THETA, taken once per
    // meta-step; every weight vector of the step (theta and the fast weights fw_1..fw_K of every task) is split under GM_W_HEADROOM x that
    // bound -- the planes of fw_k are written by the reduction that produces fw_k, before its own maximum could be known.  A weight that
    // outgrows theta's largest by that factor inside one inner loop turns into inf / NaN losses, which the caller sees.
    unsigned* wam = nullptr; const float* theta = nullptr;
    unsigned* viol = nullptr;                                               // the step's violation word (gm_bound.h)
    bool w_bound(const float* params, int l, gm_bound& bd) const {
        bd = gm_no_bound();
        if (!wam || !(index_of(params) || params == theta)) return false;
        bd.amax = wam + (int64_t)l * GM_BOUND_PAD; bd.stride = 0; bd.gain = nullptr; bd.hgain = GM_W_HEADROOM; bd.viol = viol;
        return true;
    }
};

// ---- The row plan of one pass of the dense schedule (DESIGN.md section 4.3 has the table of knobs x pass kind).  plan_pass decides it, once, when gcn_forward
// starts; gcn_forward executes it and leaves it in GcnCtx::plan, where head_loss and EVERY gcn_backward over the pass read it, whoever calls them and however much
// later (the second backward of the last support pass runs long after its forward: the plan is never derived again)
// PASS_PLAIN: a stand-alone pass (gm_gcn_forward, the passes the sparse backward differentiates): every row formed, nothing fused.  PASS_FWD_ONLY: nobody differentiates
// it (the query evaluations of the inner steps, finetuning's query passes, gm_proto_predict): all anyone reads is H_L at the centre rows.  PASS_DIFF: the dense backward
// differentiates it (the support passes, the last query evaluation): head + loss + gcn_backward follow
enum PassKind { PASS_PLAIN = 0, PASS_FWD_ONLY = 1, PASS_DIFF = 2 };
// How the pass leaves bufA (= dQ_L) for the head/loss launch and the gcn_backward(skip_head = 1) that follow.  DQ_MEMSET: untouched, head_loss zero-fills it with a
// memset launch; DQ_ZEROED: the last forward GEMM zero-fills it on its way out; DQ_CENTRE (GM_DEAD_ROWS): left alone -- the head/loss launch assigns its centre rows
// and the two readers of dQ_L in the backward take every other row as zeros (dZ GEMM: gm_batch::d_dq_tab; weight gradient: gm_wgrad_args::g_keep)
enum DqFill { DQ_MEMSET, DQ_ZEROED, DQ_CENTRE };
// One aggregate-first layer of a pass (a multiply-first layer forms and stores every row and only ever sets relu_bits).
//  split: the update runs on the split-bf16 kernel.
//  fuse: ... and takes the fused aggregate + GEMM: the aggregate of a row with one or two sources is formed in the GEMM's A feeders (same fma order), only rows of other
//    degrees go through a partial aggregate launch and HBM; Z_l of the other rows is never written -- where the pass is differentiated, the weight gradient forms them from
//    the same per-row source table (gm_wgrad_args::fuse2).  Same floats as the unfused pass, bit for bit.
//  formed (GM_DEAD_ROWS=3 / 4): the rows of Z_l this pass forms and the fused loader fetches -- the observable ones; Z[l] is unwritten everywhere else.  Every tile and
//    every MFMA is still issued, no product and no sum that reaches a stored value is dropped or reordered:
//     * the fused loaders read Z_l / H_{l-1} through gm_batch::d_fwd_tab (d_fwd_tab_feat), which sends every unobservable row to the zero row: they never touch a
//       row this pass did not write;
//     * the partial aggregate launches form the observable rows only (s_out = gm_batch::d_obs: +-1, keep_signed -- the scale is exactly the 1 the launch applies
//       without it; flagged rows stop at their descriptor, agg.hip: agg_unobservable).
//    Always ROWS_ALL without `fuse` (plan_check).  In a differentiated pass (GM_DEAD_ROWS=4) EVERY backward reads Z_l through the same table.
//  stored: the rows of H_l the update stores; every row is computed.  ROWS_CENTRE, last layer: only the head reads H_L, and only its centre rows (h[to_fetch]; the backward
//    takes relu' from the bits and the weight gradient from Z_L).  ROWS_SRC, below the last: H_l is read through the edges only (the next layer's aggregate, the fused
//    loaders, the table-formed weight gradient; the backward takes relu' from the bits) -- a row without an out-edge is nobody's source.  ROWS_E1, below a restricted
//    last layer: only a source of a centre's in-edge is the source of an edge anyone walks (a subset of ROWS_SRC).
//  relu_bits: the layer writes its relu' bits M[l] (where the context has them): every pass but the ones nobody differentiates
//  list (GM_AGG_OBS_LIST): the partial aggregate launch of a restricted fused layer walks the batch's compact list of its observable rows (gm_batch::obs; take == 2:
//    nothing to launch) instead of every listed row's descriptor; NULL: today's launch
//  dead_tiles (GM_DEAD_TILES): the update of a forward-only fused layer that stores the centre rows or the sources of their in-edges takes the batch's tile flags of that
//    set: a tile without a stored row issues its MFMAs on zero registers -- no table fetch, no operand load, no LDS traffic, no barrier, no epilogue (gemm_split.h)
struct LayerPlan { bool split, fuse; RowSet formed, stored; bool relu_bits; const gm_batch::obs_list* list; bool dead_tiles, pack_rows; };      // pack_rows (GM_PACK_ROWS): with dead_tiles, the set's packed tiles in the flags' place
// The pass: its kind, its layers, dQ_L, and what a gcn_backward(skip_head = 1) over it may do (GM_DEAD_ROWS=2; plan_backward, which resolves these against skip_head, has the bitwise argument).  t_centre: dQ_L is
// left to its centre rows and the zero block behind T_L is there -- the dZ GEMM stores T_L's centre rows only, the transposed aggregate reads T_L through gm_batch::d_ect.
// dq_e1: ... and the layer below is the first, aggregate-first, with a table-fed three-piece weight gradient: that aggregate stores only the rows of dQ_{L-1} that can be non-zero
// t_list: ... and walks the compact list of those rows (gm_batch::obs[2]), as LayerPlan::list
// t_dead_tiles (GM_DEAD_TILES): the table-read dZ launch under t_centre takes the centre rows' tile flags, as LayerPlan::dead_tiles
struct PassPlan { PassKind kind; LayerPlan layer[GM_MAX_GCN]; DqFill dq; bool t_centre, dq_e1; const gm_batch::obs_list* t_list; bool t_dead_tiles, t_pack_rows; };      // t_pack_rows: as LayerPlan::pack_rows, for the dZ launch

struct GcnCtx {
    const gm_batch* b; gm_layout L;
    PlaneDir* pd;                // non-NULL inside gm_meta_step
    bool is_support = false;     // gm_meta_step's support-chain context (the serial dependency of the step; the query contexts carry the bulk work)
    PassPlan plan = {};          // of the last gcn_forward over this context (all zeros before the first: PASS_PLAIN, every row, DQ_MEMSET)
    bool t_zero = false;         // GM_DEAD_ROWS=2: this call zeroed the block behind T_L (t_zero_fill), the last layer's backward may read T_L through gm_batch::d_ect
    float* Z[GM_MAX_GCN]; float* H[GM_MAX_GCN]; float* X0; float* bufA; float* bufB; float* partial;
    float* partial_l[GM_MAX_GCN];    // dense backward: own partials for the layers above the first, whose reductions are held back and run
    gm_wgrad_hold hold;              // together with the first layer's (one launch less per layer and backward pass)
    uint16_t* Wsplit;            // per-task weights of the GEMM being launched as three bf16 planes (split-bf16 kernel, gemm_split.h)
    float* WTl[GM_MAX_GCN];      // per-task transposed weights of layer l >= 1, [set][fo][fi]: B of the dZ GEMM (dense backward)
    const float* wt_of[GM_MAX_GCN]; int64_t wt_stride[GM_MAX_GCN];      // the parameter vector (pointer, per-set stride) WTl[l] is the transpose of
    uint8_t* M[GM_MAX_GCN];      // packed relu' bits of H[l] (one byte per 4 columns): what the backward reads instead of H[l] (dense schedule)
    float* cG2; float* cT2; float* cG1; float* partial_c;      // compact matrices of the row-sparse backward
    float* Pool; float* Gpool; float* ro_part;                 // mean readout (L.readout): pooled rows P [subs, Hd] (the head's compact input), their gradient G [subs, Hd], chunk partials
    const float* x0_user; const int32_t* centre; int z1_valid;
    int zw[GM_MAX_GCN];
    const gm_cone* cone;       // non-NULL: receptive-field schedule, every buffer is compact (gm_hparams_t.cone)
    SgdK sgd;                  // next != NULL: the backward also writes the SGD-updated parameters (inner loop)
    // Two-piece fp16 split kernels (np == 2, gm_meta_step's dense schedule; gm_bound.h): per-pass slots am[pass][2 Lg + 1][sets] (zeroed once per
    // meta-step) receive the per-set maxima of H_l (forward GEMM epilogues), T_l (dZ GEMM epilogues) and dQ_L (head backward); hv / tv / dqv:
    // recorded in the current pass.  A launch whose bounds are not all there runs the three-piece bf16 kernels.
    int hub_set = 0;           // which of the batch's two hub counter / partial-row sets this context's aggregate launches use (gm_batch_hub_alt)
    int np = 3; unsigned* am = nullptr; int am_passes = 0, am_pass = -1;
    const unsigned* feat_bound = nullptr;      // [sets] per-task bound of the layer-1 operand: the largest |feature| of the graphs the task draws from (NULL: loose table, three-piece)
    bool hv[GM_MAX_GCN] = {}, tv[GM_MAX_GCN] = {}; bool dqv = false;
    unsigned* am_slot(int i) const { return am + ((int64_t)am_pass * (2 * L.n_gcn + 1) + i) * b->sets * GM_BOUND_PAD; }
    unsigned* amH(int l) const { return am_slot(l); }
    unsigned* amT(int l) const { return am_slot(L.n_gcn + l); }
    unsigned* amdQ() const { return am_slot(2 * L.n_gcn); }
};
// bound of Z_l, the aggregate of layer l's input (features or H_{l-1}): the A operand of the forward GEMM and of the weight gradient
static bool in_bound(const GcnCtx& c, int l, gm_bound& bd) {
    bd = gm_no_bound();
    if (c.np != 2 || c.am_pass < 0 || !c.b->d_gain) return false;
    if (l == 0) {
        if (c.x0_user || !c.feat_bound) return false;
        bd.amax = c.feat_bound; bd.stride = 1;
    } else {
        if (!c.hv[l - 1]) return false;
        bd.amax = c.amH(l - 1); bd.stride = GM_BOUND_PAD;
    }
    bd.gain = c.b->d_gain; bd.hgain = 1.f;
    return true;
}
// bound of dQ_l (the gradient at layer l's output): from the head for the last layer, else relu' * norm * A^T T_{l+1}
static bool dq_bound(const GcnCtx& c, int l, gm_bound& bd) {
    bd = gm_no_bound();
    if (c.np != 2 || c.am_pass < 0 || !c.b->d_gain) return false;
    if (l == c.L.n_gcn - 1) { if (!c.dqv) return false; bd.amax = c.amdQ(); bd.gain = nullptr; }
    else { if (!c.tv[l + 1]) return false; bd.amax = c.amT(l + 1); bd.gain = c.b->d_gain + 1; }
    bd.stride = GM_BOUND_PAD; bd.hgain = 1.f;
    return true;
}
// The weight operand of a split GEMM of layer l (o = 0: X @ W, A bound in_bound; 1: dQ @ W^T, A bound dq_bound) and both bounds, into g: the planes a reduction left for
// `params`, else split now into c.Wsplit.  Two pieces where the launch has its A bound and the weights theirs (such a launch records its output's maximum), else three
static int weight_planes(GcnCtx& c, const float* params, int64_t pstride, int l, int o, hipStream_t st, gm_gemm_args& g) {
    const int fi = c.L.dims[l], fo = c.L.dims[l + 1];
    const bool want16 = o ? dq_bound(c, l, g.a_bound) : in_bound(c, l, g.a_bound);
    uint16_t* have = (c.pd && pstride) ? c.pd->lookup(params, l, o) : nullptr;       // left by the reduction that wrote these weights
    g.b_bound = gm_no_bound(); g.np = 3; g.bsplit_stride = pstride ? (int64_t)3 * fi * fo : 0;
    if (have && c.np == 2) {                                               // stored planes are two-piece in this context
        if (want16 && c.pd->w_bound(params, l, g.b_bound)) g.np = 2; else have = nullptr;
    }
    if (!have) {
        if (want16 && c.pd && c.pd->w_bound(params, l, g.b_bound)) g.np = 2; else g.b_bound = gm_no_bound();
        GM_TRY(gm_split_weights(params, pstride, c.L.w_off[l], o ? fo : fi, o ? fi : fo, o, pstride ? c.b->sets : 1, c.Wsplit, st, g.np, g.b_bound));
        have = c.Wsplit;
    }
    g.Bsplit = have;
    if (g.np == 2) { g.amax_out = o ? c.amT(l) : c.amH(l); (o ? c.tv : c.hv)[l] = true; }
    return GM_OK;
}

// Mean readout (gm_set_readout; kernels and launchers at the end of this file): the batch's chunk tables, P = mean rows of H_L, dQ_L from G
static bool mean_readout(const GcnCtx& c) { return c.L.readout == GM_READOUT_MEAN; }
static int64_t readout_chunk_count(const gm_batch* b);
static int readout_tables(const gm_batch* b, hipStream_t s);
static int readout_fwd(const GcnCtx& c, hipStream_t st);
static int readout_bwd(const GcnCtx& c, hipStream_t st);

// What layer l's weight gradient writes, in every schedule: its shape, the partials, dW_l / db_l inside `dparams`, and the context's fused SGD step
static void wgrad_out(gm_wgrad_args& w, const GcnCtx& c, int l, float* partial, float* dparams, int64_t dstride) {
    w.K = c.L.dims[l]; w.N = c.L.dims[l + 1]; w.partial = partial;
    w.dW = dparams + c.L.w_off[l]; w.dw_stride = dstride; w.db = dparams + c.L.b_off[l]; w.db_stride = dstride;
    w.sgd_cur = c.sgd.cur; w.sgd_cur_stride = c.sgd.cur_stride; w.sgd_next = c.sgd.next; w.sgd_next_stride = c.sgd.next_stride; w.sgd_lr = c.sgd.lr;
    w.w_off = c.L.w_off[l]; w.b_off = c.L.b_off[l];
}

static void gcn_carve(GcnCtx& c, Carver& cv) {
    const gm_layout& L = c.L; const int64_t rows = c.b->rows;
    int maxd = 0; int64_t maxkn = 0;
    if (c.cone) {
        const gm_cone* cn = c.cone;
        int64_t maxn = 1; int maxc = 1;
        for (int l = 0; l <= L.n_gcn; ++l) { maxn = std::max<int64_t>(maxn, cn->lv[l].n); maxc = std::max(maxc, cn->lv[l].n_chunks); }
        for (int l = 0; l < L.n_gcn; ++l) {
            const int fi = L.dims[l], fo = L.dims[l + 1];
            c.zw[l] = fi > fo ? fo : fi;
            c.Z[l] = cv.take<float>((int64_t)(fi > fo ? cn->lv[l].n : cn->lv[l + 1].n) * c.zw[l]);   // multiply-first: Y lives on the source level
            c.H[l] = cv.take<float>((int64_t)cn->lv[l + 1].n * fo);
            maxd = std::max(maxd, std::max(fi, fo));
            maxkn = std::max<int64_t>(maxkn, (int64_t)(fi + 1) * fo);
        }
        c.X0 = (L.dims[0] > L.dims[1]) ? cv.take<float>((int64_t)cn->lv[0].n * L.dims[0]) : nullptr;
        c.bufA = cv.take<float>(maxn * maxd);
        c.bufB = cv.take<float>(maxn * maxd);
        c.partial = cv.take<float>((int64_t)maxc * maxkn);
        c.cG2 = c.cT2 = c.cG1 = c.partial_c = nullptr;
        return;
    }
    for (int l = 0; l < L.n_gcn; ++l) {
        const int fi = L.dims[l], fo = L.dims[l + 1];
        c.zw[l] = fi > fo ? fo : fi;
        c.Z[l] = cv.take<float>(rows * c.zw[l]);
        c.H[l] = cv.take<float>(rows * fo);
        c.M[l] = (fo % 4 == 0 && l + 1 < L.n_gcn) ? cv.take<uint8_t>(rows * fo / 4) : nullptr;
        maxd = std::max(maxd, std::max(fi, fo));
        maxkn = std::max<int64_t>(maxkn, (int64_t)(fi + 1) * fo);
    }
    c.X0 = (L.dims[0] > L.dims[1]) ? cv.take<float>(rows * L.dims[0]) : nullptr;
    c.bufA = cv.take<float>(rows * maxd);
    c.bufB = cv.take<float>((rows + GM_ZERO_ROWS) * maxd);      // T of the dense backward + the zero block behind T_L (t_zero_rows)
    c.partial = cv.take<float>((int64_t)c.b->n_chunks * maxkn);
    for (int l = 1; l < L.n_gcn; ++l) c.partial_l[l] = cv.take<float>((int64_t)c.b->n_chunks * (L.dims[l] + 1) * L.dims[l + 1]);
    for (int l = 1; l < L.n_gcn; ++l) c.WTl[l] = cv.take<float>((int64_t)c.b->sets * L.dims[l] * L.dims[l + 1]);
    c.Wsplit = cv.take<uint16_t>((int64_t)c.b->sets * 3 * maxd * maxd);
    c.cG2 = cv.take<float>((int64_t)c.b->n_c * maxd); c.cT2 = cv.take<float>((int64_t)c.b->n_c * maxd);
    c.cG1 = cv.take<float>((int64_t)c.b->n_e1 * maxd);
    c.partial_c = cv.take<float>((int64_t)std::max(c.b->n_c_chunks, c.b->n_e1_chunks) * maxkn);
    if (mean_readout(c)) {
        const int64_t pooled = (int64_t)c.b->subs * L.dims[L.n_gcn];
        c.Pool = cv.take<float>(pooled); c.Gpool = cv.take<float>(pooled); c.ro_part = cv.take<float>(readout_chunk_count(c.b) * L.dims[L.n_gcn]);
    }
}

extern "C" int64_t gm_gcn_ws_bytes(const gm_batch_t* b, const gm_model_t* m) {
    GcnCtx c{}; c.b = b;
    if (!b || gm_make_layout(m, &c.L) != GM_OK) return -1;
    Carver cv(nullptr, 0);
    gcn_carve(c, cv);
    return cv.used + 256;
}

// > 0: every set of the batch holds this many subgraphs (HeadK::subs_per_set)
static int head_subs_per_set(const gm_batch* b) {
    int n = b->sets > 0 ? b->subs / b->sets : 0;
    for (int t = 0; t <= b->sets && n; ++t) if (b->h_set_sub_off[t] != t * n) n = 0;
    return n;
}
static HeadK make_head(const GcnCtx& c, const float* params, int64_t pstride) {
    const gm_layout& L = c.L; const gm_batch* b = c.b;
    HeadK k{};
    k.H = c.H[L.n_gcn - 1]; k.ldh = L.dims[L.n_gcn]; k.Hd = L.dims[L.n_gcn];
    k.sub_off = b->d_sub_off; k.centre = c.centre ? c.centre : b->d_centre; k.nc = b->centres; k.sub_set = b->d_sub_set;
    k.set_sub_off = b->d_set_sub_off; k.params = params; k.pstride = pstride; k.wl_off = L.wl_off; k.bl_off = L.bl_off;
    k.hc = L.hc; k.C = L.n_out; k.subs = b->subs; k.compact = c.cone ? 1 : 0;
    if (mean_readout(c)) { k.H = c.Pool; k.compact = 1; k.nc = 1; }      // the pooled rows, one per subgraph (pairs too): hc = Hd
    k.dq_amax = (c.np == 2 && c.am_pass >= 0) ? c.amdQ() : nullptr;
    k.subs_per_set = head_subs_per_set(b);
    return k;
}
static int launch_head_fwd(const GcnCtx& c, const float* params, int64_t pstride, float* logits, hipStream_t st) {
    hipLaunchKernelGGL(k_head_fwd, dim3((c.b->subs + 3) / 4), dim3(256), 0, st, make_head(c, params, pstride), logits);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
// dQ: the full-height dQ_L (zero-filled by the caller), or Gc: its centre rows as a compact matrix
static int launch_head_bwd(GcnCtx& c, const float* params, int64_t pstride, const float* dlogits, float* dparams, int64_t dstride, float* dQ, float* Gc, hipStream_t st) {
    const HeadK k = make_head(c, params, pstride);
    hipLaunchKernelGGL(k_head_bwd, dim3(c.b->sets), dim3(256), 0, st, k, dlogits, dparams, dstride, dQ, Gc);
    GM_HIP(hipGetLastError());
    if (dQ && k.dq_amax) c.dqv = true;
    return GM_OK;
}

// One aggregate launch under the launch accounting: `bytes` as SURVEY 8(d) prices it, `strict_bytes` its compulsory HBM part
static int launch_agg(const gm_agg_args& a, int64_t bytes, int64_t strict_bytes, hipStream_t st) {
    gm_prof_agg_begin(st, bytes); gm_prof_note(GM_PROF_AGG_STRICT, strict_bytes);
    const int rc = gm_launch_aggregate(a, st);
    gm_prof_agg_end(st);
    return rc;
}
// ---- The launch builders (declared, with what each is for, in gm_internal.h): every schedule below and every gm_dense_* export of dense_exports.hip fills these field
// groups through them and nowhere else
void agg_graph(const gm_batch* b, int dir, gm_agg_args& a) {
    a = gm_agg_args{};
    if (dir == 0) { a.indptr = b->d_indptr; a.indices = b->d_indices; } else { a.indptr = b->d_indptr_t; a.indices = b->d_indices_t; }
    a.heavy = b->d_heavy[dir]; a.n_heavy = b->n_heavy[dir]; a.heavy_deg = b->heavy_deg;
    a.rows = b->rows;
    // weighted batches: an aggregate without a source scale still carries the edges' weights (the callers that scale by the source's norm replace this
    // with d_enorm, which holds weight x norm).  A pointer choice only: the kernels read e_w as they do on unweighted batches
    if (b->weighted) a.e_w = b->d_ew[dir];
}
int batch_agg(const gm_batch* b, int dir, int hub_set, hipStream_t st, gm_agg_args& a) {
    agg_graph(b, dir, a);
    a.sched = b->d_sched[dir]; a.sched_len = b->sched_len[dir]; a.sched_win = b->sched_win;
    return gm_agg_hub(a, b, dir, st, hub_set);
}
void agg_take_list(gm_agg_args& a, const gm_batch::obs_list& ol) {
    a.rowlist = ol.rows; a.n_list = ol.cap; a.n_list_dev = ol.len; a.list_win = ol.win;
    a.sched = ol.sched; a.sched_len = ol.sched ? ol.sched_len : 0; a.sched_win = ol.win;
}
void agg_centre_t(gm_agg_args& a, const gm_batch* b, RowSet out) {
    a.x_idx = b->d_ect;
    if (out != ROWS_ALL) { a.s_out = row_view(b, out, false).keep; a.keep_signed = 1; }
}
LevelView batch_level(const gm_batch* b) { return {b->d_norm, b->d_tiles, b->n_tiles, b->d_chunks, b->d_set_chunk_off, b->n_chunks, b->rows, b->sets}; }
void gemm_rows(gm_gemm_args& g, const LevelView& v) { g.row_scale = v.norm; g.tiles = v.tiles; g.n_tiles = v.n_tiles; g.rows = v.rows; }
void wgrad_rows(gm_wgrad_args& w, const LevelView& v) {
    w.a_scale = v.norm; w.chunks = v.chunks; w.n_chunks = v.n_chunks; w.set_chunk_off = v.set_chunk_off; w.sets = v.sets; w.rows = v.rows;
}
void gemm_keep_rows(gm_gemm_args& g, const RowView& v, bool keep, bool live, int64_t n_keep, bool pack) {
    if (keep) { g.row_scale_keep = v.keep; g.n_keep = n_keep; }
    if (live) g.tile_live = v.live;
    if (live && pack) g.pack = v.pack;
}
void gemm_dq_table(gm_gemm_args& g, const gm_batch* b, const float* dQ, int64_t ld) { g.fuse2 = b->d_dq_tab; g.zside = dQ; g.ldz = ld; }
RowView row_view(const gm_batch* b, RowSet rs, bool gather) {
    if (rs == ROWS_E1) return {b->d_norm_e1, b->d_obs[1], gather ? b->d_fwd_tab_feat : b->d_fwd_tab[1], 1, b->n_e1, b->d_tile_live[1], b->pack[1].tiles ? &b->pack[1] : nullptr};
    if (rs == ROWS_CENTRE) return {b->d_norm_c, b->d_obs[0], b->d_fwd_tab[0], 0, b->n_c, b->d_tile_live[0], b->pack[0].tiles ? &b->pack[0] : nullptr};
    return {rs == ROWS_SRC ? b->d_norm_src : nullptr, nullptr, gather ? b->d_fuse2_feat : b->d_fuse2, -1, rs == ROWS_SRC ? b->n_src : b->rows, nullptr, nullptr};
}
// Rows of a set, and the by-source edges of those rows, for the launch accounting: exact when it is on (ROWS_E1: read back / counted once per batch at first use, which
// synchronises the stream), their bounds otherwise -- nobody reads them then
static int64_t rows_kept(const gm_batch* b, RowSet rs, hipStream_t st) { return rs != ROWS_E1 ? row_view(b, rs, false).n : gm_prof_enabled() ? gm_batch_e1_rows(b, st) : std::min<int64_t>(b->n_e1, b->rows); }

// What the partial aggregate launch of a fused layer moves (only the rows the fused kernel does not form itself: more than GM_FUSE_MAXDEG sources; of those, under
// GM_DEAD_ROWS=3 / 4, the `formed` ones -- the others stop at their descriptor): *bytes as SURVEY 8(d) prices B_agg, *strict its compulsory HBM part
static int partial_agg_bytes(const gm_batch* b, RowSet formed, int fi, bool gather, hipStream_t st, int64_t* bytes, int64_t* strict) {
    // w = {rows written, their in-edges, their distinct sources}: read once and written once (the high-degree rows of a subgraph reach ~all of its rows).  Counted once
    // per batch when the launch accounting is on, their bounds otherwise -- nobody reads them then
    const bool all = formed == ROWS_ALL;
    int64_t w[3] = {std::min<int64_t>(b->unfused_rows, row_view(b, formed, gather).n), b->unfused_edges, std::min<int64_t>(b->unfused_edges, b->rows)};
    if (gm_prof_enabled() && all) w[2] = gm_batch_unfused_sources(b, st);
    if (gm_prof_enabled() && !all) GM_TRY(gm_batch_fwd_counts(b, row_view(b, formed, gather).obs, st, w));
    // every indptr entry; the norm of every row of more than GM_FUSE_MAXDEG sources (a restricted launch: its list entry and its flag); the edge-table entries of the
    // rows written and those rows
    // (GM_AGG_OBS_LIST: a launch over the set's own list is priced like the descriptor walk it replaces -- an upper bound on its index traffic; the row, edge and
    // source terms, which carry the width, are the same either way)
    const int64_t pb0 = 4 * (b->rows + 1) + (all ? 4 : 8) * b->unfused_rows + 4 * w[1] + 4 * w[0] * (int64_t)fi;
    *bytes = pb0 + 4 * w[2] * (int64_t)fi;
    // strict HBM pricing as for the full launches: a gather launch reads at most the whole (cache-resident) feature table
    *strict = pb0 + 4 * (gather ? std::min<int64_t>(w[2], b->feat_rows) : w[2]) * (int64_t)fi;
    gm_prof_note(GM_PROF_AGG_BOUND, pb0 + 4 * std::min<int64_t>(w[1], b->rows) * (int64_t)fi - *bytes);      // (difference of the sources' bound to their exact count)
    return GM_OK;
}
// ... and the last layer's transposed aggregate of a t_centre backward (PassPlan), which works on n_out rows with e_out edges (every other row leaves behind its
// descriptor): every indptr entry and every row scale; of the rows it works on the edge-table entries and the relu' bits; T_L's centre rows read once, the rows it
// stores written once
// (GM_AGG_OBS_LIST: priced the same over the rows' own list, as partial_agg_bytes)
static int64_t t_centre_agg_bytes(const gm_batch* b, RowSet out, int fi, bool maskbits, hipStream_t st) {
    const int64_t n_out = rows_kept(b, out, st), e_out = (out == ROWS_E1 && gm_prof_enabled()) ? gm_batch_e1_edges(b, st) : b->edges;
    return 4 * (b->rows + 1) + 4 * b->rows + 4 * e_out + (maskbits ? n_out * (int64_t)fi / 4 : 0) + 4 * ((int64_t)b->n_c + n_out) * (int64_t)fi;
}

// The dZ GEMM of layer l >= 1 (dQ_l @ W_l^T: K = fo, N = fi) runs on the split kernels ...
static bool dz_split_ok(const GcnCtx& c, int l) { return c.Wsplit && gm_gemm_split_ok(c.b->n_tiles, c.L.dims[l + 1], c.L.dims[l]); }
// ... and on their fused loader, which reads a dQ_l that holds its centre rows only through the batch's table (DQ_CENTRE): plan_pass leaves dQ_L unfilled
// only where this holds
static bool dz_centre_ok(const GcnCtx& c, int l) { return dz_split_ok(c, l) && c.L.dims[l + 1] >= 64 && c.L.dims[l + 1] <= 4096 && c.b->d_dq_tab; }
// GM_DEAD_ROWS=2: the zero block behind T_L = rows [rows, rows + GM_ZERO_ROWS) of bufB at T_L's width -- where gm_batch::d_ect sends every edge whose destination is
// not a centre.  NULL where there is none: one GCN layer, the cone schedule, or a layer below the last whose T is wider than T_L and would run over the block.
// Zeroed once per call that owns the workspace (t_zero_fill, where the context's last dZ GEMM can take the table-read launch at all): no launch writes a row of
// T past `rows`.  GcnCtx::t_zero says that this call filled it -- gcn_backward reads T_L through d_ect only then
static float* t_zero_rows(const GcnCtx& c) {
    const gm_layout& L = c.L; const int Lg = L.n_gcn;
    if (c.cone || Lg < 2 || !c.bufB || L.dims[Lg - 1] > L.dims[Lg]) return nullptr;
    for (int l = 0; l < Lg - 1; ++l) if (std::min(L.dims[l], L.dims[l + 1]) > L.dims[Lg - 1]) return nullptr;
    return c.bufB + c.b->rows * (int64_t)L.dims[Lg - 1];
}
// The GM_DEAD_ROWS level in force for this context: GM_CENTRE_STORE=0 ("every row stored") switches every level off, and so do user-supplied centres (the batch's
// tables are built over its own)
static int dead_row_level(const GcnCtx& c) { return (gm_knob().centre_store == 0 || c.centre) ? 0 : gm_knob().dead_rows; }
static int t_zero_fill(GcnCtx& c, hipStream_t st) {
    float* z = t_zero_rows(c);
    c.t_zero = z && dead_row_level(c) >= 2 && dz_centre_ok(c, c.L.n_gcn - 1) && c.b->d_ect && c.b->d_norm_e1;
    if (c.t_zero) GM_HIP(hipMemsetAsync(z, 0, sizeof(float) * GM_ZERO_ROWS * c.L.dims[c.L.n_gcn - 1], st));
    return GM_OK;
}

// ================================================================================ row-sparse backward
static bool sparse_bwd_ok(const gm_layout& L) {
    if (L.n_gcn > 2 || L.readout == GM_READOUT_MEAN) return false;      // (mean readout: dQ_L is dense, every row reaches the head)
    for (int l = 0; l < L.n_gcn; ++l) if (L.dims[l] > L.dims[l + 1]) return false;      // aggregate-first layers only
    return true;
}
// dW_l = sum_k norm[r_k] Z_l[r_k]^T G[k] ; db_l = sum_k G[k] over the compact rows k of level v, whose batch rows are a_row (a set without any gets zeros: empty chunk range)
static int sparse_wgrad(GcnCtx& c, int l, const LevelView& v, const int32_t* a_row, const float* G, float* dparams, int64_t dstride, hipStream_t st) {
    gm_wgrad_args w{}; wgrad_out(w, c, l, c.partial_c, dparams, dstride); wgrad_rows(w, v);
    w.A = c.Z[l]; w.lda = w.K; w.a_row = a_row; w.G = G; w.ldg = w.N;
    return gm_launch_wgrad(w, st);
}
// Exact row-sparse backward (see gm_hparams_t.sparse_bwd).  The head is the only consumer of the last GCN layer, so
// dQ_L lives on the centre rows; one transposed-aggregate step spreads it along the in-edges of the centres.  Every
// product below is the dense backward's product with the structurally-zero terms removed.
static int gcn_backward_sparse(GcnCtx& c, const float* params, int64_t pstride, const float* dlogits, float* dparams, int64_t dstride, hipStream_t st, int skip_head) {
    const gm_layout& L = c.L; const gm_batch* b = c.b;
    const int Lg = L.n_gcn, fiL = L.dims[Lg - 1], foL = L.dims[Lg];
    // the two compact levels: the centre rows k (batch row c_k), and the centres' in-edges e (source u_e), which no GEMM runs over
    const LevelView lc = {b->d_cnorm, b->d_c_tiles, b->n_c_tiles, b->d_c_chunks, b->d_c_set_chunk_off, b->n_c_chunks, b->n_c, b->sets};
    const LevelView le = {b->d_e1_norm, nullptr, 0, b->d_e1_chunks, b->d_e1_set_chunk_off, b->n_e1_chunks, b->n_e1, b->sets};
    if (!skip_head) GM_TRY(launch_head_bwd(c, params, pstride, dlogits, dparams, dstride, nullptr, c.cG2, st));
    GM_TRY(sparse_wgrad(c, Lg - 1, lc, b->d_crow, c.cG2, dparams, dstride, st));
    if (Lg == 1) return GM_OK;
    // T2[k] = norm[c_k] * (G2[k] W_L^T)
    gm_gemm_args g{}; g.A = c.cG2; g.lda = foL; g.B = params + L.w_off[Lg - 1]; g.b_stride = pstride; g.transB = 1; g.C = c.cT2; g.ldc = fiL; g.K = foL; g.N = fiL;
    gemm_rows(g, lc);
    GM_TRY(gm_launch_gemm_nn(g, st));
    if (b->n_e1 > 0) {
        const int64_t tot = (int64_t)b->n_e1 * fiL;
        hipLaunchKernelGGL(k_expand_edges, dim3((int)std::min<int64_t>(2048, (tot + 255) / 256)), dim3(256), 0, st, c.cT2, c.H[0], fiL, b->d_e1_row, b->d_e1_par,
                           b->weighted ? b->d_e1_coef : b->d_e1_norm, b->n_e1, c.cG1);      // (weighted batches: the edge's weight rides in the coefficient)
        GM_HIP(hipGetLastError());
    }
    return sparse_wgrad(c, 0, le, b->d_e1_row, c.cG1, dparams, dstride, st);
}

// ================================================================================ receptive-field ("cone") schedule
// The same layer formulas as gcn_forward/gcn_backward, evaluated only on the rows that can reach a centre
// (cone.hip): layer l maps level l (sources) to level l+1 (destinations); all matrices are compact.

// SURVEY 8(d)'s B_agg on the rows a level-to-level aggregate actually touches: the destination level's row bounds + norms, the edges between the
// two levels, every source-level row read once (by construction each of them is the source of at least one of those edges), every
// destination row written once
static int64_t cone_agg_bytes(int64_t n_dst, int64_t n_src, int64_t nnz, int width) {
    return 4 * (n_dst + 1) + 4 * nnz + 4 * n_dst + 4 * (n_src + n_dst) * (int64_t)width;
}
static int cone_launch_agg(const gm_agg_args& a, int64_t n_src, int64_t nnz, hipStream_t st) {
    const int64_t by = cone_agg_bytes(a.rows, n_src, nnz, a.width);
    return launch_agg(a, by, by, st);
}
static gm_agg_args cone_agg(const gm_cone* cn, const gm_cone_level& up, int transposed) {
    gm_agg_args a{};
    a.indptr = transposed ? up.d_indptr_t : up.d_indptr; a.indices = transposed ? up.d_indices_t : up.d_indices;
    a.heavy = up.d_heavy[transposed]; a.n_heavy = up.n_heavy[transposed]; a.heavy_deg = cn->heavy_deg;
    a.e_w = transposed ? up.d_ew_t : up.d_ew;      // weighted batches (NULL otherwise): the edges' weights; launches that scale by the source's norm take d_enorm / d_enorm_t instead
    return a;
}
// a level of the cone as the GEMMs and weight gradients over its rows take it
static LevelView cone_level(const gm_cone_level& v, int sets) { return {v.d_norm, v.d_tiles, v.n_tiles, v.d_chunks, v.d_set_chunk_off, v.n_chunks, v.n, sets}; }

static int cone_forward(GcnCtx& c, const float* params, int64_t pstride, float* logits, hipStream_t st, int reuse_z1, int skip_head) {
    const gm_layout& L = c.L; const gm_batch* b = c.b; const gm_cone* cn = c.cone;
    GM_TRY(gm_check_feat_dim(b, L.dims[0], "forward"));
    GM_REQUIRE((L.link != 0) == (b->centres == 2), GM_EINVAL, "forward: link_pred model needs a 2-centre batch and vice versa");
    GM_REQUIRE(!c.x0_user && !c.centre, GM_EINVAL, "forward: the cone schedule reads features and centres from the batch");
    const float* xin = nullptr;
    for (int l = 0; l < L.n_gcn; ++l) {
        const gm_cone_level& lo = cn->lv[l]; const gm_cone_level& up = cn->lv[l + 1];
        const int fi = L.dims[l], fo = L.dims[l + 1];
        if (fi > fo) {                      // multiply on the source level, then aggregate into the destination level
            const float* A = xin;
            if (l == 0) { GM_TRY(gm_gather_rows(b, lo.d_feat_row, lo.n, fi, c.X0, st)); A = c.X0; }
            gm_gemm_args g{}; g.A = A; g.lda = fi; g.B = params + L.w_off[l]; g.b_stride = pstride; g.C = c.Z[l]; g.ldc = fo; g.K = fi; g.N = fo;
            gemm_rows(g, cone_level(lo, b->sets));
            GM_TRY(gm_launch_gemm_nn(g, st));
            gm_agg_args a = cone_agg(cn, up, 0);
            a.x = c.Z[l]; a.ldx = fo; a.s_out = up.d_norm; a.bias = params + L.b_off[l]; a.bias_stride = pstride; a.set_row_off = up.d_set_off; a.n_sets = b->sets;
            a.relu = 1; a.out = c.H[l]; a.rows = up.n; a.width = fo;
            GM_TRY(cone_launch_agg(a, lo.n, up.nnz, st));
        } else {
            if (!(l == 0 && reuse_z1 && c.z1_valid)) {
                gm_agg_args a = cone_agg(cn, up, 0);
                a.s_in = lo.d_norm; a.e_w = up.d_enorm; a.out = c.Z[l]; a.rows = up.n; a.width = fi; a.ldx = fi;
                if (l == 0) { a.x = b->feat; a.x_row = lo.d_feat_row; a.x_idx = up.d_efeat; a.ldx = b->feat_ld; } else a.x = xin;
                GM_TRY(cone_launch_agg(a, lo.n, up.nnz, st));
                if (l == 0) c.z1_valid = 1;
            }
            gm_gemm_args g{}; g.A = c.Z[l]; g.lda = fi; g.B = params + L.w_off[l]; g.b_stride = pstride; g.C = c.H[l]; g.ldc = fo; g.K = fi; g.N = fo;
            g.bias = params + L.b_off[l]; g.bias_stride = pstride; g.relu = 1; gemm_rows(g, cone_level(up, b->sets));
            GM_TRY(gm_launch_gemm_nn(g, st));
        }
        xin = c.H[l];
    }
    return skip_head ? GM_OK : launch_head_fwd(c, params, pstride, logits, st);
}

static int cone_backward(GcnCtx& c, const float* params, int64_t pstride, const float* dlogits, float* dparams, int64_t dstride, hipStream_t st, int skip_head) {
    const gm_layout& L = c.L; const gm_batch* b = c.b; const gm_cone* cn = c.cone;
    const int Lg = L.n_gcn;
    float* dQ = c.bufA; float* T = c.bufB;
    if (!skip_head) GM_TRY(launch_head_bwd(c, params, pstride, dlogits, dparams, dstride, nullptr, dQ, st));   // dQ_L on the centre rows
    for (int l = Lg - 1; l >= 0; --l) {
        const gm_cone_level& lo = cn->lv[l]; const gm_cone_level& up = cn->lv[l + 1];
        const int fi = L.dims[l], fo = L.dims[l + 1];
        const float* maskprev = l > 0 ? c.H[l - 1] : nullptr;
        gm_wgrad_args w{}; wgrad_out(w, c, l, c.partial, dparams, dstride);
        if (fi > fo) {
            // dY = A^T (norm * dQ) on the source level ; dW = (norm*X)^T dY ; db = colsum(dQ) ; dQ_prev = relu'(H_prev) * norm * (dY W^T)
            gm_agg_args a = cone_agg(cn, up, 1);
            a.x = dQ; a.ldx = fo; a.s_in = up.d_norm; a.e_w = up.d_enorm_t; a.out = T; a.rows = lo.n; a.width = fo;
            GM_TRY(cone_launch_agg(a, up.n, up.nnz, st));
            w.A = l > 0 ? c.H[l - 1] : c.X0; w.lda = fi; w.G = T; w.ldg = fo; w.db = nullptr; wgrad_rows(w, cone_level(lo, b->sets));
            GM_TRY(gm_launch_wgrad(w, st));
            hipLaunchKernelGGL(k_colsum_rows, dim3(b->sets), dim3(256), 0, st, dQ, (int64_t)fo, fo, up.d_set_off, dparams + L.b_off[l], dstride, c.sgd, L.b_off[l]);
            GM_HIP(hipGetLastError());
            if (l > 0) {
                gm_gemm_args g{}; g.A = T; g.lda = fo; g.B = params + L.w_off[l]; g.b_stride = pstride; g.transB = 1; g.C = dQ; g.ldc = fi; g.K = fo; g.N = fi;
                g.mask_h = maskprev; gemm_rows(g, cone_level(lo, b->sets));
                GM_TRY(gm_launch_gemm_nn(g, st));
            }
        } else {
            // dW = (norm*Z)^T dQ ; db = colsum(dQ) ; dZ = norm * (dQ W^T) ; dQ_prev = relu'(H_prev) * norm * A^T dZ
            w.A = c.Z[l]; w.lda = fi; w.G = dQ; w.ldg = fo; wgrad_rows(w, cone_level(up, b->sets));
            GM_TRY(gm_launch_wgrad(w, st));
            if (l > 0) {
                gm_gemm_args g{}; g.A = dQ; g.lda = fo; g.B = params + L.w_off[l]; g.b_stride = pstride; g.transB = 1; g.C = T; g.ldc = fi; g.K = fo; g.N = fi;
                gemm_rows(g, cone_level(up, b->sets));
                GM_TRY(gm_launch_gemm_nn(g, st));
                gm_agg_args a = cone_agg(cn, up, 1);
                a.x = T; a.ldx = fi; a.s_out = lo.d_norm; a.mask_h = maskprev; a.out = dQ; a.rows = lo.n; a.width = fi;
                GM_TRY(cone_launch_agg(a, up.n, up.nnz, st));
            }
        }
    }
    return GM_OK;
}


// ================================================================================ dense schedule
// gm_set_fuse_agg: the run-time switch of the fused aggregate + GEMM
static std::atomic<int> g_fuse_agg_override{-1};
extern "C" void gm_set_fuse_agg(int32_t on) { g_fuse_agg_override.store(on < 0 ? -1 : (on ? 1 : 0), std::memory_order_relaxed); }
extern "C" int32_t gm_get_fuse_agg(void) { const int o = g_fuse_agg_override.load(std::memory_order_relaxed); return o >= 0 ? o : gm_knob().fuse_agg; }

// What the executors rely on without looking again
static int plan_check(const GcnCtx& c, const PassPlan& p) {
    for (int l = 0; l < c.L.n_gcn; ++l) {
        GM_REQUIRE(p.layer[l].formed == ROWS_ALL || p.layer[l].fuse, GM_EINVAL, "plan: layer %d is formed on a row set but not fused: nothing reads it through the set's table", l);
        GM_REQUIRE(p.layer[l].formed != ROWS_CENTRE || (l == c.L.n_gcn - 1 && p.layer[l].stored == ROWS_CENTRE && (l > 0 || c.x0_user)), GM_EINVAL, "plan: layer %d is formed on the centre rows, but is not a last layer that stores them alone and reads no feature table", l);
    }
    GM_REQUIRE(!(p.kind == PASS_DIFF && p.layer[c.L.n_gcn - 1].formed == ROWS_CENTRE) || p.dq == DQ_CENTRE, GM_EINVAL, "plan: a restricted differentiated pass must leave dQ to its centre rows");
    GM_REQUIRE(!p.dq_e1 || p.t_centre, GM_EINVAL, "plan: dQ_{L-1} on the sources of the centres' in-edges needs T_L on its centre rows");
    return GM_OK;
}
// The plan of one pass (PassPlan): reads the knobs, the layout, the batch's table pointers and the context; launches nothing.  The only place of the dense path that
// reads GM_DEAD_ROWS / GM_CENTRE_STORE (through dead_row_level too), GM_FUSE_DIFF and gm_get_fuse_agg
static int plan_pass(const GcnCtx& c, const float* params, int64_t pstride, PassKind kind, int reuse_z1, PassPlan* plan) {
    const gm_layout& L = c.L; const gm_batch* b = c.b;
    const int Lg = L.n_gcn, last = Lg - 1, level = dead_row_level(c), centre_store = gm_knob().centre_store;
    const bool mean = mean_readout(c);      // every row of H_L is stored, dQ_L is written whole by the backward readout: no centre-row store, no dQ fill
    auto agg_first = [&](int l) { return L.dims[l] <= L.dims[l + 1]; };      // learner.py:41-47 (else learner.py:34-40: multiply first, then aggregate)
    auto wgrad_tabled = [&](int l) { return gm_wgrad_gather_ok(b->n_chunks, L.dims[l], L.dims[l + 1]); };      // the weight gradient's split kernel can form Z_l's rows from a table
    PassPlan p{}; p.kind = kind; p.dq = DQ_MEMSET;
    for (int l = 0; l < Lg; ++l) {
        LayerPlan& lp = p.layer[l]; const int fi = L.dims[l];      // (formed = stored = ROWS_ALL)
        lp.relu_bits = !agg_first(l) || kind != PASS_FWD_ONLY;
        if (!agg_first(l)) continue;
        lp.split = c.Wsplit && gm_gemm_split_ok(b->n_tiles, fi, L.dims[l + 1]) && ((uintptr_t)(params + L.b_off[l]) & 15) == 0 && pstride % 4 == 0;
        const bool gather = (l == 0 && !c.x0_user);
        // the fused aggregate + GEMM: in the passes nobody differentiates and, round 6, in the passes that ARE differentiated by the dense backward: their only
        // other reader of Z_l is the weight gradient, whose split kernel forms the same rows from the same table (gm_wgrad_gather_ok; three-piece
        // arithmetic only) -- the differentiated passes no longer write and re-read Z_l either (GM_FUSE_DIFF=0: as before)
        // GM_FUSE_DIFF=2: ... except where the pass's full launches would take the stream aggregate (a support batch with stream tables, agg_stream.hip):
        // that kernel runs INSIDE the CUs the query stream's GEMM occupies, a partial window launch competes with it for them
        const bool keeps_stream = gm_knob().fuse_diff == 2 && c.is_support && gm_knob().agg_stream && gm_stream_batch_ok(b, 0);
        const bool diff_ok = kind == PASS_DIFF && gm_knob().fuse_diff && !keeps_stream && c.np != 2 && !c.cone && wgrad_tabled(l);
        lp.fuse = (kind == PASS_FWD_ONLY || diff_ok) && gm_get_fuse_agg() && lp.split && !(l == 0 && reuse_z1) && fi >= 64 && fi % 4 == 0 && b->d_fuse2 && b->d_enorm[0] &&
                  (!gather || (b->feat_ld % 4 == 0 && b->feat_ld >= fi)) &&
                  // worth it only where a good part of the rows has one or two sources: on dense batches (Tissue shape: ~30 in-edges per
                  // row) nearly every row still goes through the ordinary aggregate and the gather feeders only cost (3.30 -> 3.21 ms)
                  2 * b->unfused_rows <= b->rows;
        // the stores of H_l (LayerPlan::stored).  GM_CENTRE_STORE: in every pass (2), in the forward-only passes (1); GM_DEAD_ROWS >= 1 below the last layer, where a
        // differentiated pass has the relu' bits to write in the stores' place
        if (l == last) { if (!mean && !c.centre && b->d_norm_c && (centre_store >= 2 || (centre_store == 1 && kind == PASS_FWD_ONLY))) lp.stored = ROWS_CENTRE; }
        else if (level >= 1 && lp.split && (kind == PASS_FWD_ONLY || (kind == PASS_DIFF && c.M[l])) && L.dims[l + 1] <= L.dims[l + 2] && b->d_norm_src) lp.stored = ROWS_SRC;
    }
    // dQ_L, decided where the last layer is aggregate-first (a multiply-first one keeps DQ_MEMSET).  The head + loss + backward follow a PASS_DIFF (gm_meta_step): the
    // last layer's GEMM zero-fills dQ on its way out instead of a memset launch.  GM_DEAD_ROWS >= 1: ... or no fill at all, where both readers of dQ_L can take the rows
    // the head/loss launch does not assign as zeros: the dZ GEMM on the fused kernel through gm_batch::d_dq_tab, the weight gradient on the three-piece split kernel
    // (gm_wgrad_args::g_keep; gcn_forward asserts that the forward launch got three pieces too)
    if (kind == PASS_DIFF && agg_first(last) && !mean)
        p.dq = (level >= 1 && p.layer[last].split && c.np != 2 && b->d_norm_c && (last == 0 || dz_centre_ok(c, last)) && wgrad_tabled(last)) ? DQ_CENTRE : DQ_ZEROED;
    // GM_DEAD_ROWS=2 (PassPlan::t_centre, dq_e1).  Deeper models than two layers keep dQ_{L-1} whole: it is the A operand of a plain-loader dZ GEMM
    p.t_centre = p.dq == DQ_CENTRE && c.t_zero && level >= 2;
    p.dq_e1 = p.t_centre && Lg == 2 && agg_first(0) && c.np != 2 && wgrad_tabled(0);
    // GM_DEAD_ROWS=3 / 4 (LayerPlan::formed): the last layer on the centre rows, the one below on the sources of the centres' in-edges.  What both levels need: the centre
    // readout, three pieces, the batch's own centres and tables, the last layer fused on the split kernel ...
    const bool last_ok = !mean && c.np != 2 && b->d_norm_c && b->d_norm_e1 && b->d_fwd_tab[0] && b->d_obs[0] && agg_first(last) && p.layer[last].fuse;
    const bool below_ok = Lg >= 2 && agg_first(Lg - 2) && b->d_fwd_tab[1] && b->d_fwd_tab_feat && b->d_obs[1];
    // Level 3: all anyone reads of a pass nobody differentiates is H_L at the centre rows, so Z_L is observable at the centre rows only, and H_{L-1} and Z_{L-1} only
    // at the sources of the centres' in-edges.  (A last layer that gathers from the feature table has no table of its own: one-layer models stay as they are.)
    const bool fwd3 = kind == PASS_FWD_ONLY && level >= 3 && centre_store >= 1 && last_ok && (Lg >= 2 || c.x0_user);
    // Level 4: a gradient reaches Z_L at the centre rows only (dQ_L is zero everywhere else) and Z_{L-1} / H_{L-1} only at the sources of the centres' in-edges
    // (dQ_{L-1} likewise), so the forward forms, fetches and stores exactly what level 3 does, and the weight gradients read Z_l through the same tables.
    // Under level 3's preconditions plus what level 2 needs of this pass -- t_centre: dQ_L left to its centre rows and the zero block behind T_L; every pass's
    // centre-row store (GM_CENTRE_STORE=2).  Not with a hoisted Z_1 (reuse_z1), which stays a flagged extra; one-layer models stay as they are.
    // The relu' bits M[l] of a restricted layer are the every-row pass's on the observable rows; on every other row they come from a zero operand row (relu'(b_l):
    // deterministic, not the every-row pass's).  Their readers: (a) the transposed aggregate behind support_bwd / the query backward (skip_head = 1, dq_e1):
    // keep_signed over d_norm_e1, it forms -- and selects by the bits of -- the observable rows only; (b) the transposed aggregate of a backward that fills dQ_L
    // itself (skip_head = 0: the meta-gradient through the last support pass) runs over every row, and on an unobservable row selects between +0 and
    // (+0 aggregate) x norm = +0: the same +0 either way.
    const bool diff4 = kind == PASS_DIFF && level >= 4 && centre_store >= 2 && p.t_centre && !reuse_z1 && Lg >= 2 && last_ok;
    if (fwd3 || diff4) p.layer[last].formed = ROWS_CENTRE;
    // The layer below.  Level 3: stored on ROWS_E1 wherever it runs on the split kernel, and formed on them where it is fused as well (not with a hoisted Z_1).  Level 4:
    // under dq_e1 (two GraphConv layers, aggregate-first, the table-fed weight gradient), fused, with the relu' bits -- a three-layer model restricts its last layer only
    if (below_ok && ((fwd3 && p.layer[Lg - 2].split) || (diff4 && p.dq_e1 && p.layer[0].fuse && c.M[0]))) {
        p.layer[Lg - 2].stored = ROWS_E1; if (p.layer[Lg - 2].fuse) p.layer[Lg - 2].formed = ROWS_E1; }
    // GM_AGG_OBS_LIST: the launches restricted above walk the batch's lists of their rows where it built and took them (finalize_finish: bound below half the rows
    // walked today, a schedule where the orientation has hub rows).  The first hub set only, as the d_mid list; the lists are over the batch's own centres, like the
    // restricted sets themselves (dead_row_level)
    if (gm_knob().agg_obs_list && c.hub_set == 0) {
        auto taken = [&](int k) { return b->obs[k].take ? &b->obs[k] : nullptr; };
        for (int l = 0; l < Lg; ++l)
            if (p.layer[l].fuse && p.layer[l].formed != ROWS_ALL) p.layer[l].list = taken(p.layer[l].formed == ROWS_CENTRE ? 0 : 1);
        if (p.dq_e1) p.t_list = taken(2);
    }
    // GM_DEAD_TILES: the fused three-piece launches that store a flagged row set and leave nothing else behind for the other rows -- a forward-only layer stored on
    // the centre rows or on the sources of their in-edges (no relu' bits, no dQ fill), and the table-read dZ launch that stores T_L's centre rows.  The last layer
    // of a PASS_DIFF writes relu' bits for every row and stays as it is
    if (gm_knob().dead_tiles) {
        for (int l = 0; l < Lg; ++l) {
            const LayerPlan& lp = p.layer[l];
            p.layer[l].dead_tiles = kind == PASS_FWD_ONLY && lp.fuse && !lp.relu_bits && c.np != 2 && (lp.stored == ROWS_CENTRE || lp.stored == ROWS_E1) &&
                                    row_view(b, lp.stored, false).live != nullptr;
        }
        p.t_dead_tiles = p.t_centre && c.np != 2 && b->d_tile_live[0] != nullptr;
        // GM_PACK_ROWS: the same launches take the set's packed tiles where the batch carries them
        if (gm_knob().pack_rows) {
            for (int l = 0; l < Lg; ++l) p.layer[l].pack_rows = p.layer[l].dead_tiles && row_view(b, p.layer[l].stored, false).pack != nullptr;
            p.t_pack_rows = p.t_dead_tiles && row_view(b, ROWS_CENTRE, false).pack != nullptr;
        }
    }
    *plan = p; return plan_check(c, p);
}

// ---- gcn_forward executes the pass's plan; one step function per launch group of a layer
// learner.py:34-40: multiply first, then aggregate (every row formed and stored; of the plan such a layer takes its relu' bits only)
static int fwd_mul_first(GcnCtx& c, int l, const float* params, int64_t pstride, const float* xin, hipStream_t st) {
    const gm_layout& L = c.L; const gm_batch* b = c.b; const int fi = L.dims[l], fo = L.dims[l + 1];
    if (l == 0 && !c.x0_user) { GM_TRY(gm_gather_rows(b, b->d_feat_row, b->rows, fi, c.X0, st)); xin = c.X0; }
    gm_gemm_args g{}; g.A = xin; g.lda = fi; g.B = params + L.w_off[l]; g.b_stride = pstride; g.C = c.Z[l]; g.ldc = fo; g.K = fi; g.N = fo;
    gemm_rows(g, batch_level(b));
    GM_TRY(gm_launch_gemm_nn(g, st));
    gm_agg_args a; GM_TRY(batch_agg(b, 0, c.hub_set, st, a));
    a.x = c.Z[l]; a.ldx = fo; a.s_out = b->d_norm;
    a.bias = params + L.b_off[l]; a.bias_stride = pstride; a.set_row_off = b->d_set_row_off; a.n_sets = b->sets; a.relu = 1;
    a.out = c.H[l]; a.width = fo; a.relu_bits = c.plan.layer[l].relu_bits ? c.M[l] : nullptr;
    return launch_agg(a, gm_aggregate_bytes(b, fo), gm_aggregate_bytes(b, fo), st);
}
// learner.py:41-47, aggregate first: Z_l = A (norm x), over x / ldx, the layer's input as the aggregate and the fused loader read it (gather: the feature table)
static int fwd_aggregate(GcnCtx& c, int l, const float* x, int64_t ldx, bool gather, hipStream_t st) {
    const gm_batch* b = c.b; const int fi = c.L.dims[l]; const LayerPlan& lp = c.plan.layer[l];
    gm_agg_args a; GM_TRY(batch_agg(b, 0, c.hub_set, st, a));
    a.s_in = b->d_norm; a.e_w = b->d_enorm[0]; a.out = c.Z[l]; a.width = fi;
    a.x = x; a.ldx = ldx; if (gather) { a.x_row = b->d_feat_row; a.x_idx = b->d_efeat; }
    if (!lp.fuse) {
        if (a.e_w) GM_TRY(gm_agg_stream_args(a, b, 0, gather, st));      // full launches may take the LDS-DMA stream kernel (agg_stream.hip)
        // compulsory HBM bytes: a gather launch reads rows of the (cache-resident) feature table, at most all of it
        int64_t strict = gm_aggregate_bytes(b, fi);
        if (gather) strict += 4 * b->rows - 4 * b->rows * (int64_t)fi + std::min<int64_t>(4 * b->rows * (int64_t)fi, 4 * b->feat_rows * (int64_t)fi);
        GM_TRY(launch_agg(a, gm_aggregate_bytes(b, fi), strict, st));
        if (l == 0) c.z1_valid = 1;
        return GM_OK;
    }
    // only the rows the fused kernel does not form itself (more than GM_FUSE_MAXDEG sources): a partial launch
    a.skip_on = 1; a.skip_lo = 0; a.skip_hi = GM_FUSE_MAXDEG;
    if (b->d_mid && c.hub_set == 0 && gm_knob().agg_mid_list && (b->n_heavy[0] == 0 || b->d_sched_mid)) {
        // ... walking the compact list of those rows (hub rows keep their blocks; the schedule is the list's)
        a.rowlist = b->d_mid; a.n_list = b->n_mid; a.list_win = b->mid_win;
        if (b->n_heavy[0] > 0) { a.sched = b->d_sched_mid; a.sched_len = b->sched_len_mid; a.sched_win = b->mid_win; }
        else { a.sched = nullptr; a.sched_len = 0; }
    }
    // ... and of those only the rows the plan forms; the others stop at their descriptor (list entry, row bounds, flag)
    if (lp.formed != ROWS_ALL) { a.s_out = row_view(b, lp.formed, gather).sign; a.keep_signed = 1; }
    // ... walking the compact list of THOSE rows where the plan took it (no launch where the host knows it empty)
    if (lp.list && lp.list->take == 2) return GM_OK;
    if (lp.list && lp.list->take == 1) agg_take_list(a, *lp.list);
    int64_t pb, pbs;
    GM_TRY(partial_agg_bytes(b, lp.formed, fi, gather, st, &pb, &pbs));
    return launch_agg(a, pb, pbs, st);
}
// ... then H_l = relu(norm Z_l W_l + b_l), on the kernel, through the loader and with the stores its plan says
static int fwd_update(GcnCtx& c, int l, const float* params, int64_t pstride, const float* x, int64_t ldx, bool gather, hipStream_t st) {
    const gm_layout& L = c.L; const gm_batch* b = c.b; const int fi = L.dims[l], fo = L.dims[l + 1];
    const LayerPlan& lp = c.plan.layer[l]; const bool last = l == L.n_gcn - 1;
    gm_gemm_args g{}; g.A = c.Z[l]; g.lda = fi; g.B = params + L.w_off[l]; g.b_stride = pstride; g.C = c.H[l]; g.ldc = fo; g.K = fi; g.N = fo;
    gemm_rows(g, batch_level(b)); g.bias = params + L.b_off[l]; g.bias_stride = pstride; g.relu = 1; g.relu_bits = lp.relu_bits ? c.M[l] : nullptr;
    // the other rows are computed, their relu' bits written, their values not stored (the kept-row count is for the launch accounting)
    if (lp.stored != ROWS_ALL) gemm_keep_rows(g, row_view(b, lp.stored, false), true, lp.dead_tiles, rows_kept(b, lp.stored, st), lp.pack_rows);
    if (lp.split) {
        GM_TRY(weight_planes(c, params, pstride, l, 0, st, g));
        GM_REQUIRE(!(last && c.plan.dq == DQ_CENTRE) || g.np == 3, GM_EINVAL, "forward: dQ is left to its centre rows, which needs the three-piece kernels");
    }
    if (last && c.plan.dq == DQ_ZEROED) g.zero_out = c.bufA;
    if (lp.fuse) { g.A = x; g.lda = ldx; g.zside = c.Z[l]; g.ldz = fi; g.fuse2 = row_view(b, lp.formed, gather).tab; }
    return gm_launch_gemm_nn(g, st);
}
// skip_head: the head (centre gather + linear) is evaluated by the fused k_head_loss launch that follows
// kind: who reads the pass (PassKind); what follows from it is plan_pass's to decide
static int gcn_forward(GcnCtx& c, const float* params, int64_t pstride, float* logits, hipStream_t st, int reuse_z1, int skip_head = 0, PassKind kind = PASS_PLAIN) {
    if (c.cone) return cone_forward(c, params, pstride, logits, st, reuse_z1, skip_head);
    const gm_layout& L = c.L; const gm_batch* b = c.b;
    if (!c.x0_user) GM_TRY(gm_check_feat_dim(b, L.dims[0], "forward"));
    GM_REQUIRE((L.link != 0) == (b->centres == 2), GM_EINVAL, "forward: link_pred model needs a 2-centre batch and vice versa");
    const float* xin = c.x0_user;           // NULL = gather rows of the store through feat_row
    GM_TRY(plan_pass(c, params, pstride, kind, reuse_z1, &c.plan));
    const bool mean = mean_readout(c);
    if (mean) GM_TRY(readout_tables(b, st));
    if (c.np == 2) {                        // a new pass: its own bound slots
        ++c.am_pass;
        GM_REQUIRE(c.am_pass < c.am_passes, GM_EINVAL, "forward: more passes than bound slots (%d)", c.am_passes);
        for (int l = 0; l < GM_MAX_GCN; ++l) c.hv[l] = c.tv[l] = false;
        c.dqv = false;
    }
    for (int l = 0; l < L.n_gcn; ++l) {
        const int fi = L.dims[l];
        if (fi > L.dims[l + 1]) GM_TRY(fwd_mul_first(c, l, params, pstride, xin, st));
        else {
            const bool gather = (l == 0 && !c.x0_user);
            const float* x = gather ? b->feat : xin; const int64_t ldx = gather ? b->feat_ld : fi;
            if (!(l == 0 && reuse_z1 && c.z1_valid)) GM_TRY(fwd_aggregate(c, l, x, ldx, gather, st));
            GM_TRY(fwd_update(c, l, params, pstride, x, ldx, gather, st));
        }
        xin = c.H[l];
    }
    if (mean) GM_TRY(readout_fwd(c, st));
    return skip_head ? GM_OK : launch_head_fwd(c, params, pstride, logits, st);
}

// ---- The plan of one gcn_backward over a pass: what the forward's plan (GcnCtx::plan, as the forward stored it: never derived again -- gm_set_fuse_agg may have changed
// since) permits, resolved against skip_head -- the one place that is done.  plan_backward decides it when gcn_backward starts; gcn_backward and its step functions execute it.
// Per aggregate-first layer l (a multiply-first one has every row of everything and no choice of kernel):
//  g_rows: the rows of dQ_l that were written -- dQ_L its centre rows, dQ_{L-1} the sources of the centres' in-edges; the other rows' bytes may be anything.  The weight
//    gradient selects zeros for them (gm_wgrad_args::g_keep)
//  dz: the kernel family of the dZ GEMM T_l = norm (dQ_l W_l^T) (DZ_NONE: the first layer has none), dz_tab: its loader reads dQ_l through gm_batch::d_dq_tab
//  t_rows: the rows of T_l that GEMM stores, t_live: ... and it takes their tile flags (GM_DEAD_TILES)
//  agg / t_ect / dq_rows / list: the transposed aggregate dQ_{l-1} = relu' norm A^T T_l launches at all (not below the first layer, not where the host knows its list
//    empty: obs_list::take == 2); reads T_l through gm_batch::d_ect; stores these rows of dQ_{l-1} (= g_rows of the layer below); walks this list of them (NULL: every row's descriptor)
// Per call, fill_dq: this call zero-fills dQ_L whole before the head writes its centre rows (neither behind head_loss nor under the mean readout, whose backward writes every row)
enum DzKind { DZ_NONE, DZ_SPLIT, DZ_WT, DZ_PLAIN };
struct BwdLayer { RowSet g_rows; DzKind dz; bool dz_tab; RowSet t_rows; bool t_live, agg, t_ect; RowSet dq_rows; const gm_batch::obs_list* list; bool t_pack; };
struct BwdPlan { bool fill_dq; BwdLayer layer[GM_MAX_GCN]; };
static int plan_backward(const GcnCtx& c, int skip_head, BwdPlan* out) {
    const gm_layout& L = c.L; const PassPlan& plan = c.plan; const int last = L.n_gcn - 1;
    BwdPlan p{}; p.fill_dq = !skip_head && !mean_readout(c);
    const bool dq_centre = skip_head && plan.dq == DQ_CENTRE;      // dQ_L holds its centre rows only (head_loss); without skip_head it is filled in this call
    // GM_DEAD_ROWS=2: the same rule one level down.  Every row of T_L = norm (dQ_L W_L^T) outside the centre rows is an exact zero, and so is every row of dQ_{L-1} =
    // relu' norm A^T T_L that is not the source of an in-edge of a centre.  Every row is still computed, no product and no sum is dropped:
    //  * the dZ GEMM stores T_L's centre rows only (row_scale_keep = d_norm_c);
    //  * the transposed aggregate reads T_L through gm_batch::d_ect, which sends an edge into any other row to the zero block behind T_L (t_zero_rows).  Bitwise the
    //    dense pass: there the row read is +-0 (a +0-started sum of +-0 products, times a positive norm), and fma(+-0, w, acc) leaves the aggregate's +0-started
    //    chain unchanged -- a +0 accumulator stays +0, any other value stays itself; the block's +0 does the same.  (A non-finite W_L makes the dense pass's zeros
    //    NaN and not these: the forward over the same weights then gave a NaN loss, and the NaN guard discards the step -- DESIGN 4.3);
    //  * where the layer below is the first, that aggregate stores only the rows of dQ_{L-1} that can be non-zero (s_out = d_norm_e1, keep_signed), and the first
    //    layer's weight gradient selects zeros for the others (g_keep).  Deeper models keep dQ_{L-1} whole: it is the A operand of a plain-loader dZ GEMM.
    const bool t_centre = dq_centre && plan.t_centre, dq_e1 = t_centre && plan.dq_e1;
    for (int l = last; l >= 0; --l) {
        const int fi = L.dims[l], fo = L.dims[l + 1];
        BwdLayer& bl = p.layer[l];
        if (fi > fo) continue;
        bl.g_rows = l == last ? (dq_centre ? ROWS_CENTRE : ROWS_ALL) : p.layer[l + 1].dq_rows;
        // The zero rows of A of a layer formed on its observable rows only (GM_DEAD_ROWS=4; always tabled: plan_check) stand in for finite rows the every-row pass multiplies
        // by zero rows of G: those rows of G must BE zeros here too -- selected (g_keep: the backward behind head_loss, whose dQ holds the observable rows only), or true
        // zeros because this very call filled dQ_L before the head wrote its centre rows (skip_head = 0: the meta-gradient through the last support pass, which runs over the
        // Z / H / M that pass's restricted forward left).  Bitwise the every-row pass in both: a +-0 product added to a chain that started at +0 leaves the chain unchanged
        // (bsum and the MFMA accumulators start at +0; a zero A row makes the same +-0 products as a finite one); in the second, dQ_L's other rows are the memset's +0, T_L's
        // are +0 x norm, the transposed aggregate's +0-started chains over them stay +0, and the relu' select yields +0 whichever way the bit reads
        GM_REQUIRE(plan.layer[l].formed == ROWS_ALL || row_view(c.b, bl.g_rows, false).keep || p.fill_dq, GM_EINVAL, "backward: layer %d was formed on its observable rows only, but its weight gradient got neither flagged rows of G (g_keep) nor a dQ this call zero-filled", l);
        if (l == 0) continue;
        bl.dz = dz_split_ok(c, l) ? DZ_SPLIT : (c.WTl[l] && fi % 64 == 0 && fo % 16 == 0) ? DZ_WT : DZ_PLAIN;
        // dQ_L with its centre rows only: the fused kernel's loader reads them through the batch's table (fma(0, 0, fma(x, 1, 0)) = x) and zeros for every other row -- the
        // same tile, bit for bit, as the plain launch over a zero-filled dQ.  (plan_pass chose DQ_CENTRE under dz_centre_ok, which holds for a context or not at all: a
        // dQ_L left to its centre rows always comes this way)
        bl.dz_tab = bl.dz == DZ_SPLIT && dq_centre && l == last;
        bl.t_rows = (bl.dz == DZ_SPLIT && t_centre && l == last) ? ROWS_CENTRE : ROWS_ALL;
        bl.t_live = bl.t_rows == ROWS_CENTRE && plan.t_dead_tiles; bl.t_pack = bl.t_live && plan.t_pack_rows;
        bl.t_ect = t_centre && l == last;
        bl.dq_rows = (bl.t_ect && dq_e1) ? ROWS_E1 : ROWS_ALL;      // the rows that launch works on (every other row leaves behind its descriptor)
        const gm_batch::obs_list* tl = bl.dq_rows == ROWS_E1 ? plan.t_list : nullptr;
        bl.list = (tl && tl->take == 1) ? tl : nullptr;
        bl.agg = !(tl && tl->take == 2);
    }
    *out = p; return GM_OK;
}

// ---- gcn_backward executes it; one step function per launch group of a layer.  w arrives with the batch's rows, the layer's outputs and its hold slot
// relu'(H_{l-1}) as layer l's backward reads it: the packed bits where the context has them (1/16 of the bytes of H_{l-1}), else H_{l-1} itself; nothing below the first layer
struct ReluMask { const float* h; const uint8_t* bits; };
static ReluMask relu_mask(const GcnCtx& c, int l) { const uint8_t* m = l > 0 ? c.M[l - 1] : nullptr; return {(l > 0 && !m) ? c.H[l - 1] : nullptr, m}; }
// multiply-first: dY = A^T (norm * dQ) ; dW = (norm*X)^T dY ; db = colsum(dQ) ; dQ_prev = relu'(H_prev) * norm * (dY W^T)
static int bwd_mul_first(GcnCtx& c, int l, gm_wgrad_args& w, const float* params, int64_t pstride, hipStream_t st) {
    const gm_layout& L = c.L; const gm_batch* b = c.b; const int fi = L.dims[l], fo = L.dims[l + 1];
    float* dQ = c.bufA; float* T = c.bufB;
    gm_agg_args a; GM_TRY(batch_agg(b, 1, c.hub_set, st, a));
    a.x = dQ; a.ldx = fo; a.s_in = b->d_norm; a.e_w = b->d_enorm[1]; a.out = T; a.width = fo;
    GM_TRY(launch_agg(a, gm_aggregate_bytes(b, fo), gm_aggregate_bytes(b, fo), st));
    w.A = l > 0 ? c.H[l - 1] : (c.x0_user ? c.x0_user : c.X0); w.lda = fi; w.G = T; w.ldg = fo; w.Gb = dQ; w.ldgb = fo;
    GM_TRY(gm_launch_wgrad(w, st));
    if (l == 0) return GM_OK;
    gm_gemm_args g{}; g.A = T; g.lda = fo; g.B = params + L.w_off[l]; g.b_stride = pstride; g.transB = 1; g.C = dQ; g.ldc = fi; g.K = fo; g.N = fi;
    const ReluMask m = relu_mask(c, l);
    gemm_rows(g, batch_level(b)); g.mask_h = m.h; g.mask_b = m.bits;
    return gm_launch_gemm_nn(g, st);
}
// aggregate-first: dW = (norm*Z)^T dQ ; db = colsum(dQ) ; dZ = norm * (dQ W^T) ; dQ_prev = relu'(H_prev) * norm * A^T dZ
// Order: dZ GEMM (reads dQ and the CURRENT weights) -> weight gradient (reads dQ; its reduction writes the updated
// weights and, for the next step's dZ GEMM, their transpose) -> transposed aggregate (overwrites dQ).
// The weight gradient's operands: G = dQ_l on the rows that were written, A = Z_l as the forward left it
static void bwd_wgrad_operands(const GcnCtx& c, int l, const BwdLayer& bl, gm_wgrad_args& w, hipStream_t st) {
    const gm_batch* b = c.b; const int fi = c.L.dims[l]; const LayerPlan& lp = c.plan.layer[l];
    w.A = c.Z[l]; w.lda = fi; w.G = c.bufA; w.ldg = c.L.dims[l + 1];
    w.g_keep = row_view(b, bl.g_rows, false).keep;
    if (lp.fuse) {            // the forward ran fused: Z[l] holds the rows of three or more sources, the table forms the others
        const bool gather = l == 0 && !c.x0_user;
        // GM_DEAD_ROWS=4: ... and of a restricted pass through the forward's own table: an unobservable row of A is the zero row -- the forward
        // wrote neither its Z_l row nor (one layer down) the H_{l-1} rows the full table would gather for it
        w.fuse2 = row_view(b, lp.formed, gather).tab;
        w.gx = gather ? b->feat : (l > 0 ? c.H[l - 1] : c.x0_user); w.ldgx = gather ? b->feat_ld : fi;
    }
    // launch accounting: A is fetched on the observable rows only (every other row reads the cache-resident zero row)
    if (lp.formed != ROWS_ALL && gm_prof_enabled()) w.a_rows = rows_kept(b, lp.formed, st);
}
// T_l = norm (dQ_l W_l^T), K = fo, N = fi, on the plan's kernel family
static int bwd_dz(GcnCtx& c, int l, const BwdLayer& bl, gm_wgrad_args& w, const float* params, int64_t pstride, hipStream_t st) {
    const gm_layout& L = c.L; const gm_batch* b = c.b; const int fi = L.dims[l], fo = L.dims[l + 1];
    gm_gemm_args g{}; g.A = c.bufA; g.lda = fo; g.C = c.bufB; g.ldc = fi; g.K = fo; g.N = fi;
    gemm_rows(g, batch_level(b));
    g.B = params + L.w_off[l]; g.b_stride = pstride; g.transB = 1;
    if (bl.dz == DZ_SPLIT) {
        // B = W^T with W stored [fi][fo]: the planes are W's own rows (no transpose)
        GM_TRY(weight_planes(c, params, pstride, l, 1, st, g));
        if (bl.dz_tab) gemm_dq_table(g, b, c.bufA, fo);
        if (bl.t_rows != ROWS_ALL) gemm_keep_rows(g, row_view(b, bl.t_rows, false), true, bl.t_live, rows_kept(b, bl.t_rows, st), bl.t_pack);
    } else if (bl.dz == DZ_WT) {
        // dZ = dQ @ W^T through the direct-to-LDS kernel on transposed weights: left there by the previous step's
        // weight-gradient reduction (which wrote these very weights), else transposed now (T x 256 KB)
        if (!(c.wt_of[l] == params && c.wt_stride[l] == pstride)) {
            const int nt = pstride ? b->sets : 1;         // shared theta (step 0): one transpose serves every task
            hipLaunchKernelGGL(k_transpose_w, dim3((fo + 31) / 32, (fi + 31) / 32, nt), dim3(256), 0, st, params, pstride, L.w_off[l], fi, fo, c.WTl[l]);
            GM_HIP(hipGetLastError());
            c.wt_of[l] = params; c.wt_stride[l] = pstride;
        }
        g.B = c.WTl[l]; g.b_stride = pstride ? (int64_t)fi * fo : 0; g.transB = 0;
        if (c.sgd.next) w.wt_next = c.WTl[l];
    }
    return gm_launch_gemm_nn(g, st);
}
// ... the weight gradient: planes of the updated weights for the next step's GEMMs, two-piece bounds, the launch, and what it left behind
static int bwd_wgrad(GcnCtx& c, int l, gm_wgrad_args& w, hipStream_t st) {
    int kn = 0;
    if (c.pd && c.sgd.next && (kn = c.pd->index_of(c.sgd.next)) != 0) { w.pl_fwd = c.pd->slot(kn, l, 0); w.pl_dz = c.pd->slot(kn, l, 1); }
    if (c.np == 2) {
        gm_bound ab, gb;
        if (in_bound(c, l, ab) && dq_bound(c, l, gb)) { w.np = 2; w.a_bound = ab; w.g_bound = gb; }
        if (kn) {                                                  // two-piece planes of the updated weights, under the step's weight bound
            if (c.pd->w_bound(c.sgd.next, l, w.pl_bound)) w.pl_np = 2; else { w.pl_fwd = nullptr; w.pl_dz = nullptr; }
        }
    }
    GM_TRY(gm_launch_wgrad(w, st));
    if (kn) { c.pd->valid[kn][l][0] = w.pl_fwd != nullptr; c.pd->valid[kn][l][1] = w.pl_dz != nullptr; }
    if (w.wt_next) { c.wt_of[l] = c.sgd.next; c.wt_stride[l] = c.sgd.next_stride; }
    return GM_OK;
}
// ... dQ_{l-1} = relu'(H_{l-1}) norm A^T T_l, overwriting dQ
static int bwd_agg_t(GcnCtx& c, int l, const BwdLayer& bl, hipStream_t st) {
    const gm_batch* b = c.b; const int fi = c.L.dims[l]; const ReluMask m = relu_mask(c, l);
    gm_agg_args a; GM_TRY(batch_agg(b, 1, c.hub_set, st, a));
    a.x = c.bufB; a.ldx = fi; a.s_out = b->d_norm; a.mask_h = m.h; a.mask_b = m.bits;
    a.out = c.bufA; a.width = fi;
    if (bl.t_ect) agg_centre_t(a, b, bl.dq_rows);
    if (bl.list) agg_take_list(a, *bl.list);
    const int64_t by = bl.t_ect ? t_centre_agg_bytes(b, bl.dq_rows, fi, m.bits != nullptr, st) : gm_aggregate_bytes(b, fi);
    return launch_agg(a, by, by, st);
}
// skip_head: dQ_L / the compact G2 and the head's own gradients were already produced by k_head_loss (head_loss below)
static int gcn_backward(GcnCtx& c, const float* params, int64_t pstride, const float* dlogits, float* dparams, int64_t dstride, hipStream_t st, int sparse = 0,
                        int skip_head = 0) {
    if (c.cone) return cone_backward(c, params, pstride, dlogits, dparams, dstride, st, skip_head);
    if (sparse && sparse_bwd_ok(c.L)) return gcn_backward_sparse(c, params, pstride, dlogits, dparams, dstride, st, skip_head);
    const gm_layout& L = c.L; const gm_batch* b = c.b;
    BwdPlan bp; GM_TRY(plan_backward(c, skip_head, &bp));
    c.hold.n = 0;
    if (!skip_head) {      // dQ_L from the head: zero-filled and its centre rows written, or -- mean readout -- G = dlogits Wl on the pooled rows, then every row from it
        if (bp.fill_dq) GM_HIP(hipMemsetAsync(c.bufA, 0, sizeof(float) * b->rows * L.dims[L.n_gcn], st));
        GM_TRY(launch_head_bwd(c, params, pstride, dlogits, dparams, dstride, bp.fill_dq ? c.bufA : nullptr, bp.fill_dq ? nullptr : c.Gpool, st));
        if (!bp.fill_dq) GM_TRY(readout_bwd(c, st));
    }
    for (int l = L.n_gcn - 1; l >= 0; --l) {
        const BwdLayer& bl = bp.layer[l];
        // the reduction (+ SGD step, weight planes) of a layer above the first is held back and launched with the first layer's: the new
        // W_l has no reader before the next forward
        gm_wgrad_args w{}; wgrad_out(w, c, l, l > 0 ? c.partial_l[l] : c.partial, dparams, dstride); wgrad_rows(w, batch_level(b));
        w.hold = &c.hold; w.hold_this = l > 0 ? 1 : 0;
        if (L.dims[l] > L.dims[l + 1]) { GM_TRY(bwd_mul_first(c, l, w, params, pstride, st)); continue; }
        bwd_wgrad_operands(c, l, bl, w, st);
        if (bl.dz != DZ_NONE) GM_TRY(bwd_dz(c, l, bl, w, params, pstride, st));
        GM_TRY(bwd_wgrad(c, l, w, st));
        if (bl.agg) GM_TRY(bwd_agg_t(c, l, bl, st));
    }
    return GM_OK;
}

extern "C" int gm_gcn_forward(const gm_batch_t* b, const gm_model_t* m, const float* params, int64_t param_stride, const float* x0,
                              const int32_t* centre_local, float* logits, void* ws, int64_t ws_bytes, void* stream) {
    GM_REQUIRE(b && m && params && logits && ws, GM_EINVAL, "gcn_forward: NULL argument");
    GcnCtx c{}; c.b = b;
    GM_TRY(gm_make_layout(m, &c.L));
    Carver cv(ws, ws_bytes);
    gcn_carve(c, cv);
    GM_REQUIRE(cv.ok(), GM_ENOMEM, "gcn_forward: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)cv.used);
    c.x0_user = x0; c.centre = centre_local;
    const int rc = gcn_forward(c, params, param_stride, logits, (hipStream_t)stream, 0);
    gm_batch_mark_use(b, (hipStream_t)stream);
    return rc;
}

extern "C" int gm_gcn_backward(const gm_batch_t* b, const gm_model_t* m, const float* params, int64_t param_stride, const float* x0,
                               const int32_t* centre_local, const float* dlogits, float* dparams, int64_t dparam_stride, void* ws,
                               int64_t ws_bytes, void* stream) {
    GM_REQUIRE(b && m && params && dlogits && dparams && ws, GM_EINVAL, "gcn_backward: NULL argument");
    GcnCtx c{}; c.b = b;
    GM_TRY(gm_make_layout(m, &c.L));
    GM_REQUIRE(dparam_stride >= c.L.P, GM_EINVAL, "gcn_backward: dparam_stride %lld < P=%lld", (long long)dparam_stride, (long long)c.L.P);
    Carver cv(ws, ws_bytes);
    gcn_carve(c, cv);
    GM_REQUIRE(cv.ok(), GM_ENOMEM, "gcn_backward: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)cv.used);
    c.x0_user = x0; c.centre = centre_local;
    const int rc = gcn_backward(c, params, param_stride, dlogits, dparams, dparam_stride, (hipStream_t)stream);
    gm_batch_mark_use(b, (hipStream_t)stream);
    return rc;
}

// ================================================================================ prototypical losses
// Host side of meta.py:32-42,60-65: sorted unique classes, rows of each class (first n_support for the
// support loss; all rows, equal counts required, for the query loss), as global subgraph ids.  Every set (task) keeps its
// own class layout -- the reference calls proto_loss_* once per task (meta.py:118-157), so a Shared dataset whose graphs
// carry different label sets, or evaluation tasks of different shapes, are fine.
struct ClassTables {
    std::vector<int32_t> rows;          // concatenated per set: [Ct_t][n_t] subgraph ids; a ragged set: [class starts (Ct_t + 1) | class rows]
    std::vector<int32_t> tab;           // [sets*3]: offset into rows, Ct_t, n_t; a ragged set: -(scored rows) in place of n_t
    int Ct = 0, n = 0;                  // maxima over the sets (LDS sizing, prototype stride); n: over the balanced sets
    bool uniform = false;               // every set: Ct classes x n rows, stored at set * Ct * n
    int qmax = 0;                       // largest scored-row count of a ragged set; 0 = every set is balanced.  Else n is rounded up so that Ct * n >= qmax
    std::vector<int32_t> labels;        // ragged mode: the sorted class labels of every set, concatenated (tab[3t + 1] each)
};

// Ragged-task mode (gm_set_ragged_classes, include/gmeta_hip.h): per calling thread, like gm_last_error and the profile counters
static thread_local int g_ragged = 0;
extern "C" void gm_set_ragged_classes(int32_t on) { g_ragged = on ? 1 : 0; }
extern "C" int32_t gm_get_ragged_classes(void) { return g_ragged; }

// Class tables in ragged-task mode.  support == NULL: the classes of a set are its own sorted labels, each with its first min(limit, count) rows
// (limit = 0: all).  support != NULL (the query side of a task): the classes are the support set's, a class may have no rows, and a label outside
// them is an error.  A set whose classes all score the same number of rows gets the balanced table entry -- and with it the balanced code path.
static int class_tables_ragged(const gm_batch* b, const int32_t* y, int limit, const ClassTables* support, ClassTables& ct) {
    ct.rows.clear(); ct.labels.clear(); ct.tab.assign((size_t)b->sets * 3, 0); ct.Ct = 0; ct.n = 0; ct.qmax = 0;
    size_t lab_off = 0;
    for (int t = 0; t < b->sets; ++t) {
        std::map<int32_t, std::vector<int32_t>> by;
        if (support) {
            const int nc = support->tab[t * 3 + 1];
            for (int c = 0; c < nc; ++c) by[support->labels[lab_off + c]];
            lab_off += nc;
            GM_REQUIRE(b->h_set_sub_off[t + 1] > b->h_set_sub_off[t], GM_EINVAL, "proto loss: task %d has no query rows", t);
            for (int s = b->h_set_sub_off[t]; s < b->h_set_sub_off[t + 1]; ++s) {
                auto it = by.find(y[s]);
                GM_REQUIRE(it != by.end(), GM_EINVAL, "proto loss: task %d has a query row of label %d, which is not among its support classes", t, y[s]);
                it->second.push_back(s);
            }
        } else {
            for (int s = b->h_set_sub_off[t]; s < b->h_set_sub_off[t + 1]; ++s) by[y[s]].push_back(s);
            GM_REQUIRE(!by.empty(), GM_EINVAL, "proto loss: set %d is empty", t);
        }
        const int nc = (int)by.size();
        GM_REQUIRE(nc <= 256, GM_ERANGE, "proto loss: set %d has %d classes, outside the kernel's range (256)", t, nc);
        int64_t q = 0; int first = -1; bool balanced = true;
        for (auto& kv : by) {
            const int c = limit > 0 ? std::min(limit, (int)kv.second.size()) : (int)kv.second.size();
            kv.second.resize(c);
            if (first < 0) first = c;
            balanced = balanced && c == first;
            q += c;
            ct.labels.push_back(kv.first);
        }
        GM_REQUIRE(q <= 8192, GM_ERANGE, "proto loss: set %d scores %lld rows, outside the kernel's range (8192)", t, (long long)q);
        ct.tab[t * 3] = (int32_t)ct.rows.size(); ct.tab[t * 3 + 1] = nc;
        ct.Ct = std::max(ct.Ct, nc);
        if (balanced) {
            ct.tab[t * 3 + 2] = first; ct.n = std::max(ct.n, first);
        } else {
            ct.tab[t * 3 + 2] = -(int32_t)q; ct.qmax = std::max(ct.qmax, (int)q);
            int32_t at = 0;
            for (auto& kv : by) { ct.rows.push_back(at); at += (int32_t)kv.second.size(); }
            ct.rows.push_back(at);
        }
        for (auto& kv : by) ct.rows.insert(ct.rows.end(), kv.second.begin(), kv.second.end());
    }
    GM_REQUIRE((int64_t)ct.Ct * ct.n <= 8192, GM_ERANGE, "proto loss: %d classes x %d rows per set is outside the kernel's range", ct.Ct, ct.n);
    ct.uniform = ct.qmax == 0;
    for (int t = 0; t < b->sets; ++t) ct.uniform = ct.uniform && ct.tab[t * 3] == t * ct.Ct * ct.n && ct.tab[t * 3 + 1] == ct.Ct && ct.tab[t * 3 + 2] == ct.n;
    if (ct.qmax) ct.n = std::max(ct.n, (ct.qmax + ct.Ct - 1) / ct.Ct);      // the kernels carve lse / A for Ct * n rows
    return GM_OK;
}

static int class_tables(const gm_batch* b, const int32_t* y, int limit, ClassTables& ct, const ClassTables* support = nullptr) {
    if (g_ragged) return class_tables_ragged(b, y, limit, support, ct);
    ct.rows.clear(); ct.tab.assign((size_t)b->sets * 3, 0); ct.Ct = 0; ct.n = 0; ct.qmax = 0;
    for (int t = 0; t < b->sets; ++t) {
        std::map<int32_t, std::vector<int32_t>> by;
        for (int s = b->h_set_sub_off[t]; s < b->h_set_sub_off[t + 1]; ++s) by[y[s]].push_back(s);
        GM_REQUIRE(!by.empty(), GM_EINVAL, "proto loss: set %d is empty", t);
        int cnt = -1;
        for (auto& kv : by) {
            int c = (int)kv.second.size();
            if (limit > 0) {
                GM_REQUIRE(c >= limit, GM_EINVAL, "proto loss: class %d of set %d has %d rows < n_support=%d (torch.stack at meta.py:42 fails)", kv.first, t, c, limit);
                c = limit;
            }
            GM_REQUIRE(cnt < 0 || cnt == c, GM_EINVAL, "proto loss: classes of set %d have unequal row counts (torch.stack at meta.py:65 fails)", t);
            cnt = c;
        }
        ct.tab[t * 3] = (int32_t)ct.rows.size(); ct.tab[t * 3 + 1] = (int32_t)by.size(); ct.tab[t * 3 + 2] = cnt;
        ct.Ct = std::max(ct.Ct, (int)by.size()); ct.n = std::max(ct.n, cnt);
        for (auto& kv : by) ct.rows.insert(ct.rows.end(), kv.second.begin(), kv.second.begin() + cnt);
    }
    GM_REQUIRE((int64_t)ct.Ct * ct.n <= 8192 && ct.Ct <= 256, GM_ERANGE, "proto loss: %d classes x %d rows per set is outside the kernel's range", ct.Ct, ct.n);
    ct.uniform = true;
    for (int t = 0; t < b->sets; ++t) ct.uniform = ct.uniform && ct.tab[t * 3] == t * ct.Ct * ct.n && ct.tab[t * 3 + 1] == ct.Ct && ct.tab[t * 3 + 2] == ct.n;
    return GM_OK;
}

static size_t proto_lds(int Ct, int n, int D, int nt = 256) {
    const size_t a = (size_t)Ct * n * Ct;
    return sizeof(float) * ((size_t)Ct * D + (size_t)Ct * n + 2 * (size_t)nt + (a <= PROTO_A_MAX ? a : 0));
}

template <bool RGK>
static int launch_proto_t(const gm_batch* b, const ProtoK& k, hipStream_t st) {
    GM_TRY(gm_func_full_lds((const void*)k_proto<RGK>));
    hipLaunchKernelGGL(k_proto<RGK>, dim3(b->sets), dim3(256), proto_lds(k.Ct, k.n, k.D), st, k);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
static int launch_proto_ragged(const gm_batch* b, const ProtoK& k, hipStream_t st);
static int launch_proto(const gm_batch* b, const ProtoK& k, bool ragged, hipStream_t st) { return ragged ? launch_proto_ragged(b, k, st) : launch_proto_t<false>(b, k, st); }

// rows + tab of a ClassTables on the device (one allocation: [rows | tab]); freed by the caller with gm_dev_free
static int upload_tables(const ClassTables& ct, int32_t** d_out, hipStream_t st) {
    *d_out = nullptr;
    int32_t* d = nullptr;
    GM_TRY(gm_alloc(&d, ct.rows.size() + ct.tab.size(), st));
    if (hipMemcpyAsync(d, ct.rows.data(), 4 * ct.rows.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d + ct.rows.size(), ct.tab.data(), 4 * ct.tab.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {             // pageable sources: complete before `ct` can go away
        gm_set_error("proto loss: class-table upload failed"); gm_dev_free(d, st); return GM_EHIP;
    }
    *d_out = d;
    return GM_OK;
}

extern "C" int gm_proto_loss_spt(const gm_batch_t* b, const float* logits, int32_t n_out, const int32_t* y, int32_t n_support, float* loss,
                                 float* acc, float* protos, float* dlogits, void* stream) {
    GM_REQUIRE(b && logits && y && loss && acc && n_support >= 1, GM_EINVAL, "proto_loss_spt: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    ClassTables ct;
    GM_TRY(class_tables(b, y, n_support, ct));
    int32_t* d_rows = nullptr;
    GM_TRY(upload_tables(ct, &d_rows, st));
    int rc = GM_OK;
    if (dlogits && hipMemsetAsync(dlogits, 0, sizeof(float) * b->subs * n_out, st) != hipSuccess) { gm_set_error("proto_loss_spt: memset failed"); rc = GM_EHIP; }
    if (rc == GM_OK) {
        ProtoK k{logits, n_out, d_rows, ct.Ct, ct.n, 0, nullptr, protos, loss, acc, 1, 0, dlogits, nullptr, 0, d_rows + ct.rows.size()};
        rc = launch_proto(b, k, ct.qmax != 0, st);
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == GM_OK) { gm_set_error("proto_loss_spt: kernel failed"); rc = GM_EHIP; }
    gm_dev_free(d_rows, st);
    return rc;
}

extern "C" int gm_proto_loss_qry(const gm_batch_t* b, const float* logits, int32_t n_out, const int32_t* y, const float* protos, int32_t c_task,
                                 float* loss, float* acc, float* dlogits, float* dprotos, void* stream) {
    GM_REQUIRE(b && logits && y && protos && loss && acc, GM_EINVAL, "proto_loss_qry: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    ClassTables ct;
    GM_TRY(class_tables(b, y, 0, ct));
    // prototypes are indexed by sorted-class position with stride c_task: EVERY set must carry exactly c_task query classes (a set with
    // fewer would be scored against another class's prototype); gm_meta_step checks support vs query class counts per task itself
    // (ragged-task mode: a set may carry fewer -- its classes are its own sorted labels, scored against its first prototypes)
    for (int t = 0; t < b->sets; ++t)
        GM_REQUIRE(g_ragged ? ct.tab[t * 3 + 1] <= c_task : ct.tab[t * 3 + 1] == c_task, GM_EINVAL,
                   "proto_loss_qry: set %d has %d query classes but the prototypes hold %d per set", t, ct.tab[t * 3 + 1], c_task);
    GM_REQUIRE(c_task <= 256 && (int64_t)c_task * ct.n <= 16384, GM_ERANGE, "proto_loss_qry: c_task=%d with %d rows per class is outside the kernel's range", c_task, ct.n);
    int32_t* d_rows = nullptr;
    GM_TRY(upload_tables(ct, &d_rows, st));
    int rc = GM_OK;
    if (dlogits && hipMemsetAsync(dlogits, 0, sizeof(float) * b->subs * n_out, st) != hipSuccess) { gm_set_error("proto_loss_qry: memset failed"); rc = GM_EHIP; }
    if (rc == GM_OK) {
        ProtoK k{logits, n_out, d_rows, c_task, ct.n, 1, protos, nullptr, loss, acc, 1, 0, dlogits, dprotos, 0, d_rows + ct.rows.size()};      // (prototype stride c_task)
        rc = launch_proto(b, k, ct.qmax != 0, st);
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == GM_OK) { gm_set_error("proto_loss_qry: kernel failed"); rc = GM_EHIP; }
    gm_dev_free(d_rows, st);
    return rc;
}

#ifdef GM_PROBES
// Probe build only (build.py --probes; include/gmeta_hip_probes.h)
static unsigned long long* g_head_dbg = nullptr;
// Phase timeline of k_head_loss (block 0, device constant clock): enable allocates 64 stamps that every later launch overwrites; out != NULL copies them
extern "C" int gm_head_loss_debug(int32_t enable, unsigned long long* out) {
    if (enable && !g_head_dbg) { GM_HIP(hipMalloc((void**)&g_head_dbg, 512)); GM_HIP(hipMemset(g_head_dbg, 0, 512)); }
    if (out && g_head_dbg) GM_HIP(hipMemcpy(out, g_head_dbg, 512, hipMemcpyDeviceToHost));
    if (!enable && g_head_dbg) { (void)hipFree(g_head_dbg); g_head_dbg = nullptr; }
    return GM_OK;
}
#else
static unsigned long long* const g_head_dbg = nullptr;      // the product library carries no probe state
#endif

// One k_head_loss launch: everything but the instantiation
struct HeadLossLaunch {
    int sets; size_t lds; HeadK hk; float* logits; ProtoK pk; int bwd; float* dparams; int64_t dstride; float* dQ; float* Gc; SgdK sg; int stage_h, proto_floats;
    int copy_out;             // 1 (gm_dense_head_loss only): a staged launch also writes its logits / dlogits to the global arrays
    int32_t* launched;        // tests, or NULL: receives {workgroup size, staged, ragged instantiation} of the kernel that was launched
};
template <int NT, bool RGK>
static int launch_head_loss_t(const HeadLossLaunch& a, hipStream_t st, bool again = false) {      // again: the probe's repeat of a launch just made -- the launch alone
    const auto k_head_loss_nt = k_head_loss<NT, RGK>;
    if (!again) GM_TRY(gm_func_full_lds((const void*)k_head_loss_nt));
    hipLaunchKernelGGL(k_head_loss_nt, dim3(a.sets), dim3(NT), a.lds, st, a.hk, a.logits, a.pk, a.bwd, a.dparams, a.dstride, a.dQ, a.Gc, a.sg, a.stage_h, a.proto_floats, a.copy_out, g_head_dbg);
    if (a.launched) { a.launched[0] = NT; a.launched[1] = a.stage_h; a.launched[2] = RGK ? 1 : 0; }
    return GM_OK;
}
template <bool RGK>
static int launch_head_loss(int nt, const HeadLossLaunch& a, hipStream_t st) {
    return nt == 256 ? launch_head_loss_t<256, RGK>(a, st) : nt == 512 ? launch_head_loss_t<512, RGK>(a, st) : launch_head_loss_t<1024, RGK>(a, st);
}
static int launch_head_loss_ragged(int nt, const HeadLossLaunch& a, hipStream_t st);
// The k_head_loss launch of a head (hk) and a loss (pk): the LDS of a set, staged or not, the workgroup size, the launcher.  Everything is decided from the launch's own
// arguments, so that gm_dense_head_loss (tests) runs these very decisions.  copy_out / launched: see HeadLossLaunch.
static int head_loss_launch(const gm_batch* b, const HeadK& hk, float* logits, const ProtoK& pk, int bwd, float* dparams, int64_t dstride, float* dQ, float* Gc,
                            const SgdK& sg, bool ragged, int copy_out, int32_t* launched, hipStream_t st) {
    const size_t proto_bytes = (proto_lds(pk.Ct, pk.n, pk.D, HL_THREADS) + 15) / 16 * 16;
    int max_subs = 0;
    for (int t = 0; t < b->sets; ++t) max_subs = std::max(max_subs, b->h_set_sub_off[t + 1] - b->h_set_sub_off[t]);
    const size_t hs_bytes = sizeof(float) * ((size_t)max_subs * hk.nc * hk.Hd + (size_t)hk.C * (hk.hc + 1) + 2 * (size_t)max_subs * hk.C +
                                             (size_t)max_subs * hk.nc + (size_t)pk.Ct * pk.n + (ragged ? (size_t)pk.Ct + 1 : 0)) + 16;      // + the centre-row scratch + the class rows (a ragged set's follow its class starts)
    const int stage_on = gm_knob().head_stage;
    const int stage_h = stage_on && proto_bytes + hs_bytes <= 150 * 1024;
    const size_t lds = proto_bytes + (stage_h ? hs_bytes : 0);
    // Workgroup size (GM_HEAD_THREADS, default 1024): one workgroup per task.  Measured: 256 threads -- which could start on a CU that a persistent
    // GEMM workgroup of the other stream fills -- lose more inside the kernel than they gain at its start (FirstMM shape 1.62 -> 1.89 ms per
    // meta-step, 4-task arxiv shard 4.59 -> 4.86; 512: 1.71 / 4.67).
    int nt = gm_knob().head_threads;
    if (nt != 256 && nt != 512) nt = 1024;
    const HeadLossLaunch hl{b->sets, lds, hk, logits, pk, bwd, dparams, dstride, dQ, Gc, bwd ? sg : SgdK{nullptr, 0, nullptr, 0, 0.f}, stage_h, (int)(proto_bytes / sizeof(float)),
                            copy_out, launched};
    if (!ragged) GM_TRY(launch_head_loss<false>(nt, hl, st));      // (first: the kernels every launch without ragged sets runs stay where they were in the code object)
    else GM_TRY(launch_head_loss_ragged(nt, hl, st));
#ifdef GM_PROBES
    // tools/head_loss_probe.py: the same launch again -- it is idempotent -- to see what a warm instruction cache / warm L2 is worth
    static const int twice = getenv("GM_HEAD_TWICE") ? atoi(getenv("GM_HEAD_TWICE")) : 0;
    if (twice && nt == 1024 && !ragged) (void)launch_head_loss_t<1024, false>(hl, st, true);
#endif
    GM_HIP(hipGetLastError());
    return GM_OK;
}
// Head forward + loss (+ head backward) in one launch (k_head_loss) after a gcn_forward(..., skip_head = 1).  With
// bwd != 0 the matching gcn_backward(..., skip_head = 1) continues from dQ_L / the compact G2 written here; c.sgd (if
// set) makes the head's own parameters take their SGD step in the same launch.
static int head_loss(GcnCtx& c, const float* params, int64_t pstride, float* logits, const ProtoK& pk, int bwd, float* dparams, int64_t dstride, int sparse,
                     hipStream_t st, bool ragged = false) {      // ragged: the class tables hold ragged sets (see ProtoK)
    const gm_batch* b = c.b; const gm_layout& L = c.L;
    float* dQ = nullptr; float* Gc = nullptr;
    const bool mean = mean_readout(c);
    if (bwd) {
        if (mean) Gc = c.Gpool;      // the pooled rows' gradient; readout_bwd below turns it into dQ_L
        else if (c.cone) Gc = c.bufA;
        else if (sparse && sparse_bwd_ok(L)) Gc = c.cG2;
        else {
            dQ = c.bufA;
            if (c.plan.dq == DQ_MEMSET) GM_HIP(hipMemsetAsync(dQ, 0, sizeof(float) * b->rows * L.dims[L.n_gcn], st));      // (DQ_CENTRE: nobody reads the rows this launch does not assign)
        }
    }
    const HeadK hk = make_head(c, params, pstride);
    gm_prof_begin(GM_PROF_HEAD, st, b->subs);
    GM_TRY(head_loss_launch(b, hk, logits, pk, bwd, dparams, dstride, dQ, Gc, c.sgd, ragged, 0, nullptr, st));
    gm_prof_end(GM_PROF_HEAD, st);
    if (bwd && dQ && hk.dq_amax) c.dqv = true;
    if (bwd && mean) GM_TRY(readout_bwd(c, st));
    return GM_OK;
}

// ================================================================================ ragged-task mode: kernels of launches that hold ragged sets
// Instantiated and defined HERE, behind everything a launch without ragged sets runs: those kernels keep the place in the code object they had before the mode existed
// (k_head_loss is pure latency; with the ragged instantiations emitted ahead of it, the same instructions measured 0.1-0.3 us per launch slower at the FirstMM shape).
static int launch_proto_ragged(const gm_batch* b, const ProtoK& k, hipStream_t st) { return launch_proto_t<true>(b, k, st); }
static int launch_head_loss_ragged(int nt, const HeadLossLaunch& a, hipStream_t st) { return launch_head_loss<true>(nt, a, st); }
// k_protos_to_dlogits for a launch with ragged sets ([class starts | class rows], see ProtoK): prototype_c = mean of the class's own row count
__global__ void k_protos_to_dlogits_ragged(const float* dprotos, const int32_t* rows, const int32_t* tab, int CtMax, int D, float* dlogits) {
    const int set = blockIdx.x, Ct = tab[set * 3 + 1], n = tab[set * 3 + 2];
    rows += tab[set * 3];
    if (n < 0) {
        const int32_t* coff = rows;
        rows += Ct + 1;
        for (int id = threadIdx.x; id < -n * D; id += blockDim.x) {
            const int q = id / D, d = id - q * D, c = ragged_class(coff, Ct, q);
            dlogits[(int64_t)rows[q] * D + d] = dprotos[((int64_t)set * CtMax + c) * D + d] / (float)(coff[c + 1] - coff[c]);
        }
        return;
    }
    for (int id = threadIdx.x; id < Ct * n * D; id += blockDim.x) {
        const int q = id / D, d = id - q * D, c = q / n;
        dlogits[(int64_t)rows[q] * D + d] = dprotos[((int64_t)set * CtMax + c) * D + d] / (float)n;
    }
}

// ================================================================================ the fused meta-step
// theta in the caller's layout -> the kernels' layout: `shift` zeros inserted at `cut` (the zero weight rows of the padded feature columns)
__global__ void k_pad_params(const float* theta, int64_t P, int64_t cut, int64_t shift, float* out) {
    for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < P + shift; id += (int64_t)gridDim.x * blockDim.x)
        out[id] = id < cut ? theta[id] : (id < cut + shift ? 0.f : theta[id - shift]);
}

// The model the kernels run: layer 1 reads the store's padded feature rows (gm_store::feat_ld columns, the extra ones zero), so W_1
// gets matching zero rows -- same sums, but the layer takes the vectorised aggregate / DMA GEMM / fast weight-gradient kernels
// whatever the dataset's feature width (50 and 5 in the reference's Tissue-PPI / FirstMM-DB configs).
// (a hop-labelled batch: its own table's width and leading dimension)
static gm_model_t internal_model(const gm_model_t* m, const gm_batch* b, int64_t* cut, int64_t* shift) {
    gm_model_t mp = *m; *cut = 0; *shift = 0;
    if (b->feat_ld != b->feat_dim && m->dims[0] == b->feat_dim) {
        mp.dims[0] = (int32_t)b->feat_ld;
        *cut = (int64_t)b->feat_dim * m->dims[1]; *shift = (int64_t)(b->feat_ld - b->feat_dim) * m->dims[1];
    }
    return mp;
}

// The query stream carries bulk, throughput-bound work; the caller's stream carries the latency-critical support chain.  A lower
// priority (a) lets support kernels win CUs when both have work and (b) gives the stream a hardware queue of its own: HIP multiplexes
// same-priority streams onto a small pool of HW queues (GPU_MAX_HW_QUEUES, default 4), and once RCCL/torch have created their streams an
// ordinary stream created here was observed to alias the caller's queue, silently serialising the whole step.
static int low_priority_stream(hipStream_t* st) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
        GM_HIP(hipStreamCreateWithPriority(st, hipStreamNonBlocking, lo));      // `lo` = least priority
    } else {
        (void)hipGetLastError();
        GM_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    }
    return GM_OK;
}

struct MetaStreams {
    hipStream_t side = nullptr, side2 = nullptr;      // query streams (side2: GM_QUERY_STREAMS = 2)
    std::vector<hipEvent_t> ev;
    int ensure(int n) {
        if (!side) GM_TRY(low_priority_stream(&side));
        if (!side2) GM_TRY(low_priority_stream(&side2));
        while ((int)ev.size() < n) { hipEvent_t e; GM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); ev.push_back(e); }
        return GM_OK;
    }
};
// One side stream / event pool / staging ring per (thread, device): a process may drive several GPUs.
static MetaStreams& meta_streams() {
    static thread_local std::map<int, MetaStreams> m;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    return m[dev];
}

// Pinned host staging for the per-step class tables: the H2D copy is truly asynchronous (no stream synchronisation in
// gm_meta_step); a slot is reused only after the copy that read it has completed (4 slots: never waits in practice).
struct StageRing {
    static const int N = 4;
    void* buf[N] = {}; size_t cap[N] = {}; hipEvent_t ev[N] = {}; bool busy[N] = {}; int next = 0;
    int acquire(size_t bytes, void** out, int* slot) {
        const int k = next; next = (next + 1) % N;
        if (busy[k]) { GM_HIP(hipEventSynchronize(ev[k])); busy[k] = false; }
        if (!ev[k]) GM_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        if (cap[k] < bytes) {
            if (buf[k]) (void)hipHostFree(buf[k]);
            buf[k] = nullptr; cap[k] = 0;
            const size_t want = std::max<size_t>(bytes * 2, 64 * 1024);
            GM_HIP(hipHostMalloc(&buf[k], want, hipHostMallocDefault));
            cap[k] = want;
        }
        *out = buf[k]; *slot = k;
        return GM_OK;
    }
    int release_after(int slot, hipStream_t st) { GM_HIP(hipEventRecord(ev[slot], st)); busy[slot] = true; return GM_OK; }
};
static StageRing& stage_ring() {
    static thread_local std::map<int, StageRing> m;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    return m[dev];
}
// `bytes` of host data to dst without a host synchronisation: a ring slot, filled by fill(slot memory), ONE asynchronous copy on st
template <class Fill>
static int stage_to_device(void* dst, size_t bytes, hipStream_t st, Fill&& fill) {
    void* h = nullptr; int slot = 0;
    StageRing& ring = stage_ring();
    GM_TRY(ring.acquire(bytes, &h, &slot));
    fill(h);
    GM_HIP(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st));
    return ring.release_after(slot, st);
}

// The support chain's part of a plan: gm_meta_step and gm_meta_adapt run the same launches on it (support_head / support_bwd below)
struct SupportPlan {
    gm_layout L; int T, K; int64_t Pp;       // Pp = P padded to 64 floats: per-task weight vectors stay 16-B aligned
    GcnCtx S;
    float *fw, *g, *logit_s, *dlog_s, *protos, *ls, *as_, *theta_p;
    PlaneDir pd;
    int64_t TP, proto_sz;               // fw holds K vectors-of-tasks fw_1..fw_K (distinct buffers: the support chain may run ahead)
    int32_t *rows_s, *tab_s;            // support class tables
    int64_t cap_s;                      // ints held by rows_s: spt->subs; ragged-task mode: + the class starts of ragged sets (at most spt->subs + T)
    int Ct, ns, uni_s = 0;              // uni_s: class layout uniform over the tasks (ProtoK::uniform)
    int qmax_s = 0;                     // ragged-task mode: largest scored-row count of a ragged set (0: none, the usual kernels)
    float* fw_k(int k) const { return fw + (int64_t)(k - 1) * TP; }      // fw_k, k = 1..K
};
struct MetaPlan : SupportPlan {
    GcnCtx Q, Q2;                            // Q2: second query context (own activations) when two query streams are used
    int nq_ctx; float *logit_q2;
    float *gq, *gp, *logit_q, *dlog_q, *dprotos, *lq, *aq;
    int32_t *rows_q, *tab_q;                      // class tables: one contiguous block [rows_s | rows_q | tab_s | tab_q | featb_s | featb_q]
    unsigned *featb_s, *featb_q;                  // [T] each: per-task bound of the layer-1 operand (fp32 bit patterns; rides in the class-table copy)
    unsigned* viol;                               // the step's violation word (gm_bound.h), zeroed with the bound slots; NULL without two-piece kernels
    int nq, uni_q = 0, qmax_q = 0;                // as Ct / ns, uni_s, qmax_s of the support side
    int64_t cap_q;                                // ints held by rows_q
    unsigned* bound_ws; int64_t bound_words;      // gm_bound.h slots of this step ([S passes | Q passes | weights]), zeroed by ONE memset; NULL: three-piece kernels
};

// split-bf16 planes of every fast-weight vector fw_1..fw_K (= fw + (k-1) * TP; dense schedule, layers the split GEMM can take): forward planes
// for every such layer, dZ planes for layers >= 1; ~1 MB per task and inner step at 128/256/256
static void plan_planes(PlaneDir& pd, const gm_layout& L, int T, int K, float* fw, int64_t TP, bool dense, Carver& cv) {
    pd = PlaneDir{};
    if (gm_gemm_mode() == 1 && dense && K < 64) {
        int64_t per_k = 0;
        for (int l = 0; l < L.n_gcn; ++l) {
            const int fi = L.dims[l], fo = L.dims[l + 1];
            pd.off[l][0] = pd.off[l][1] = -1;
            if (fi > fo) continue;                                           // multiply-first layers keep the on-the-fly path
            const int64_t sz = (int64_t)T * 3 * fi * fo;
            if ((fo == 256 || fo == 128) && fi % 16 == 0 && fi >= 32) { pd.off[l][0] = per_k; per_k += sz; }                 // X @ W: K = fi, N = fo
            if (l > 0 && (fi == 256 || fi == 128) && fo % 16 == 0 && fo >= 32) { pd.off[l][1] = per_k; per_k += sz; }        // dQ @ W^T: K = fo, N = fi
        }
        if (per_k > 0) {
            pd.base = cv.take<uint16_t>(per_k * K); pd.per_k = per_k; pd.fw0 = fw; pd.TP = TP; pd.K = K;
            if (!pd.base) pd.base = reinterpret_cast<uint16_t*>(1);      // sizing pass (no workspace yet): keep the layout decisions identical
        }
    }
}

// A fresh context on batch b; under hp->cone with the batch's receptive-field tables (built on first use, cached in the batch)
static int plan_ctx(GcnCtx& c, const gm_batch* b, const gm_layout& L, const gm_hparams_t* hp) {
    c = GcnCtx{}; c.b = b; c.L = L;
    if (hp->cone && L.readout != GM_READOUT_MEAN) {      // (mean readout: every row reaches the head, the dense schedule runs)
        const gm_cone* cn = nullptr;
        GM_TRY(gm_batch_cone(b, L.n_gcn, b->stream, &cn));
        if (cn->ok) c.cone = cn;         // else: a self pair among the centres -> dense schedule
    }
    return GM_OK;
}
// What every plan starts with: the layout of the model the kernels run, Pp, the context of its (first) batch
static int plan_prologue(const gm_model_t* m, const gm_hparams_t* hp, const gm_batch* b, gm_layout& L, int64_t& Pp, GcnCtx& c) {
    GM_TRY(gm_make_layout(m, &L));
    GM_TRY(gm_check_feat_dim(b, L.dims[0], "model"));      // (m: the internal model -- dims[0] is the caller's, or the padded width where the caller's matched)
    Pp = (L.P + 63) / 64 * 64;
    return plan_ctx(c, b, L, hp);
}
static int support_prologue(SupportPlan& p, const gm_batch* spt, const gm_model_t* m, const gm_hparams_t* hp) {
    GM_TRY(plan_prologue(m, hp, spt, p.L, p.Pp, p.S));
    p.S.is_support = true;
    p.T = spt->sets; p.K = hp->update_step; p.TP = (int64_t)p.T * p.Pp; p.proto_sz = (int64_t)p.T * 256 * p.L.n_out;
    return GM_OK;
}

// theta in the caller's layout (P floats) -> the kernels' (internal_model) in p.theta_p; *theta moves there
static int pad_theta(const SupportPlan& p, const float** theta, int64_t P, int64_t cut, int64_t shift, hipStream_t st) {
    if (!shift) return GM_OK;
    hipLaunchKernelGGL(k_pad_params, dim3((int)std::min<int64_t>(512, (p.L.P + 255) / 256)), dim3(256), 0, st, *theta, P, cut, shift, p.theta_p);
    GM_HIP(hipGetLastError());
    *theta = p.theta_p;
    return GM_OK;
}

// One support step (meta.py:122-126,145-151) on st, in two halves -- gm_meta_step enqueues query work between them:
//   support_head: forward -> [head + proto_loss_spt + head backward, one launch]; step k's losses go to column k, its prototypes to `protos`
//   support_bwd:  backward, with the SGD step w_next = w - lr * grad written by the kernels that produce each gradient
// w_next == NULL: the forward and the prototypes only, no support_bwd follows (gm_meta_adapt with K = 0).
static int support_head(SupportPlan& p, const gm_hparams_t* hp, int k, const float* w, int64_t wstride, float* w_next, float* protos, hipStream_t st) {
    const int bwd = w_next ? 1 : 0, sparse = hp->sparse_bwd;
    GM_TRY(gcn_forward(p.S, w, wstride, p.logit_s, st, hp->hoist_z1, 1, (sparse && sparse_bwd_ok(p.L)) ? PASS_PLAIN : PASS_DIFF));
    if (bwd) p.S.sgd = SgdK{w, wstride, w_next, p.Pp, hp->update_lr};
    ProtoK pk{p.logit_s, p.L.n_out, p.rows_s, p.Ct, p.ns, 0, nullptr, protos, p.ls, p.as_, p.K + 1, k, bwd ? p.dlog_s : nullptr, nullptr, 0, p.tab_s, p.uni_s};
    return head_loss(p.S, w, wstride, p.logit_s, pk, bwd, p.g, p.Pp, sparse, st, p.qmax_s != 0);
}
static int support_bwd(SupportPlan& p, const gm_hparams_t* hp, const float* w, int64_t wstride, hipStream_t st) {
    GM_TRY(gcn_backward(p.S, w, wstride, p.dlog_s, p.g, p.Pp, st, hp->sparse_bwd, 1));
    p.S.sgd = SgdK{nullptr, 0, nullptr, 0, 0.f};
    return GM_OK;
}

static int meta_plan(MetaPlan& p, const gm_batch* spt, const gm_batch* qry, const gm_model_t* m, const gm_hparams_t* hp, void* ws, int64_t ws_bytes,
                     int Ct, int ns, int nq, int64_t* need) {
    GM_TRY(support_prologue(p, spt, m, hp));
    GM_TRY(plan_ctx(p.Q, qry, p.L, hp));
    if (!p.S.cone || !p.Q.cone) p.S.cone = p.Q.cone = nullptr;      // one schedule for the whole step
    p.Q2 = p.Q;
    Carver cv(ws, ws_bytes);
    const int64_t TP = p.TP; const int C = p.L.n_out; const int K1 = p.K + 1;
    p.theta_p = cv.take<float>(p.Pp);
    p.fw = cv.take<float>(TP * p.K); p.g = cv.take<float>(TP); p.gq = cv.take<float>(TP); p.gp = cv.take<float>(TP);
    p.logit_s = cv.take<float>((int64_t)spt->subs * C); p.logit_q = cv.take<float>((int64_t)qry->subs * C);
    p.dlog_s = cv.take<float>((int64_t)spt->subs * C); p.dlog_q = cv.take<float>((int64_t)qry->subs * C);
    p.protos = cv.take<float>(p.proto_sz * p.K); p.dprotos = cv.take<float>(p.proto_sz);
    p.ls = cv.take<float>((int64_t)p.T * K1); p.as_ = cv.take<float>((int64_t)p.T * K1);
    p.lq = cv.take<float>((int64_t)p.T * K1); p.aq = cv.take<float>((int64_t)p.T * K1);
    {   // rows of a set never exceed its subgraphs: [rows_s (spt->subs) | rows_q (qry->subs) | tab_s (3T) | tab_q (3T)]
        // ragged-task mode: a ragged set's rows follow its class starts, one more than it has classes -- on either side at most the support set's subgraphs + 1
        const int64_t starts = g_ragged ? (int64_t)spt->subs + p.T : 0;
        p.cap_s = spt->subs + starts; p.cap_q = qry->subs + starts;
        int32_t* blk = cv.take<int32_t>(p.cap_s + p.cap_q + 8 * (int64_t)p.T);
        p.rows_s = blk; p.rows_q = blk ? blk + p.cap_s : nullptr;
        p.tab_s = blk ? p.rows_q + p.cap_q : nullptr; p.tab_q = blk ? p.tab_s + 3 * p.T : nullptr;
        p.featb_s = blk ? reinterpret_cast<unsigned*>(p.tab_q + 3 * p.T) : nullptr; p.featb_q = blk ? p.featb_s + p.T : nullptr;
    }
    // Two query streams (GM_QUERY_STREAMS=2, off by default): evaluations k and k + 1 are independent of each other (each needs only fw_k and the
    // prototypes of step k - 1), so they can run in two contexts on two streams.  Measured: no gain anywhere -- 4-task arxiv shard 4.68 vs 4.67 ms,
    // 8 tasks 8.22 vs 8.07, Tissue shape 3.46 vs 3.55, FirstMM shape 1.61 vs 1.66, task_num 32 28.09 vs 28.17 (same box): kernels of
    // different queues time-slice the chip, they do not fill each other's stalls.  Kept as a knob (bitwise the one-stream result; tested).
    {
        const int qs = gm_knob().query_streams;
        p.nq_ctx = (hp->serialize || hp->cone || hp->sparse_bwd) ? 1 : (qs == 2 ? 2 : 1);
    }
    p.logit_q2 = p.nq_ctx == 2 ? cv.take<float>((int64_t)qry->subs * C) : nullptr;
    gcn_carve(p.S, cv); gcn_carve(p.Q, cv);
    if (p.nq_ctx == 2) { gcn_carve(p.Q2, cv); p.Q2.hub_set = 1; }
    plan_planes(p.pd, p.L, p.T, p.K, p.fw, TP, !p.S.cone, cv);
    // two-piece fp16 split kernels: when the weight planes are kept, every GCN layer is aggregate-first and the dense schedule runs
    p.bound_ws = nullptr; p.bound_words = 0; p.viol = nullptr;
    bool agg_first = true;
    for (int l = 0; l < p.L.n_gcn; ++l) agg_first = agg_first && p.L.dims[l] <= p.L.dims[l + 1];
    // (never on weighted batches: the magnitude bounds -- k_gains, gm_bound.h -- assume edge scales <= 1; they keep the three-piece kernels, violation word 0)
    // (nor on hop-labelled batches: the layer-1 operand bound -- the store's largest |feature| -- does not cover the 1.0 label entries)
    // (nor under the mean readout: dQ_L comes from the readout's backward kernel, which records no bound)
    if (p.pd.base && gm_split_np() == 2 && agg_first && !hp->sparse_bwd && !p.S.cone && p.L.readout != GM_READOUT_MEAN && spt->store->d_feat_amax && !spt->weighted && !qry->weighted && !spt->hop_D && !qry->hop_D &&
        spt->rows + qry->rows >= gm_knob().split16_min_rows) {
        const int per_pass = 2 * p.L.n_gcn + 1;
        const int64_t ws_s = (int64_t)p.K * per_pass * p.T * GM_BOUND_PAD, ws_q = (int64_t)K1 * per_pass * p.T * GM_BOUND_PAD, ws_w = (int64_t)p.L.n_gcn * GM_BOUND_PAD;
        p.bound_words = ws_s + ws_q + ws_w + GM_BOUND_PAD;                   // (+ the violation word, on a line of its own)
        p.bound_ws = cv.take<unsigned>(p.bound_words);
        if (!p.bound_ws) p.bound_ws = reinterpret_cast<unsigned*>(16);       // sizing pass
        p.S.np = p.Q.np = p.Q2.np = 2;
        p.S.am = p.bound_ws; p.S.am_passes = p.K; p.Q.am = p.bound_ws + ws_s; p.Q.am_passes = K1;
        p.Q2.am = p.Q.am; p.Q2.am_passes = K1;       // (the two query contexts share the slot array: evaluation j uses pass j, set by the step)
        p.pd.wam = p.bound_ws + ws_s + ws_q;
        p.viol = p.pd.wam + ws_w; p.pd.viol = p.viol;
    }
    p.Ct = Ct; p.ns = ns; p.nq = nq;
    if (need) *need = cv.used + 256;
    GM_REQUIRE(cv.ok(), GM_ENOMEM, "meta_step: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)cv.used);
    return GM_OK;
}

extern "C" int64_t gm_meta_ws_bytes(const gm_batch_t* spt, const gm_batch_t* qry, const gm_model_t* m, const gm_hparams_t* hp) {
    if (!spt || !qry || !m || !hp) return -1;
    MetaPlan p; int64_t need = 0, cut, shift;
    const gm_model_t mp = internal_model(m, spt, &cut, &shift);
    if (meta_plan(p, spt, qry, &mp, hp, nullptr, 0, 1, 1, 1, &need) != GM_OK) return -1;
    return need;
}

extern "C" int64_t gm_meta_out_floats(const gm_batch_t* spt, const gm_model_t* m, const gm_hparams_t* hp) {
    gm_layout L;
    if (!spt || !hp || gm_make_layout(m, &L) != GM_OK) return -1;
    return L.P + 2 * (int64_t)(hp->update_step + 1) + 1 + (int64_t)spt->sets * (hp->update_step + 1) + 1;
}

extern "C" int gm_meta_step(const gm_batch_t* spt, const gm_batch_t* qry, const int32_t* y_spt, const int32_t* y_qry, const gm_model_t* m,
                            const gm_hparams_t* hp, const float* theta, float* out, int64_t out_floats, void* ws, int64_t ws_bytes, void* stream) {
    GM_REQUIRE(spt && qry && y_spt && y_qry && m && hp && theta && out && ws, GM_EINVAL, "meta_step: NULL argument");
    GM_REQUIRE(out_floats >= gm_meta_out_floats(spt, m, hp), GM_ENOMEM, "meta_step: out holds %lld floats, the step writes %lld", (long long)out_floats,
               (long long)gm_meta_out_floats(spt, m, hp));
    GM_REQUIRE(spt->sets == qry->sets, GM_EINVAL, "meta_step: %d support sets but %d query sets", spt->sets, qry->sets);
    GM_REQUIRE(spt->store == qry->store, GM_EINVAL, "meta_step: support and query batches come from different stores");
    GM_REQUIRE(spt->weighted == qry->weighted, GM_EINVAL, "meta_step: one of the support and query batches is weighted, the other is not");
    GM_REQUIRE(spt->hop_D == qry->hop_D, GM_EINVAL, "meta_step: the support batch has hop labels D=%d but the query batch D=%d", spt->hop_D, qry->hop_D);
    const int K = hp->update_step;
    GM_REQUIRE(K >= 1, GM_EINVAL, "meta_step: update_step must be >= 1");
    GM_REQUIRE(!hp->need_meta_grad || K >= 2, GM_EINVAL,
               "meta_step: update_step must be >= 2 for training (losses_q[0..1] are computed under no_grad, meta.py:129-141)");
    GM_REQUIRE(((uintptr_t)theta & 15) == 0, GM_EINVAL, "meta_step: theta must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    gm_phase_timer tm("meta_step");
    ClassTables cs, cq;
    GM_TRY(class_tables(spt, y_spt, hp->k_spt, cs));
    GM_TRY(class_tables(qry, y_qry, 0, cq, &cs));      // (ragged-task mode: the query rows are filed under the support classes, which their labels must be among)
    for (int t = 0; t < spt->sets; ++t)
        GM_REQUIRE(cs.tab[t * 3 + 1] == cq.tab[t * 3 + 1], GM_EINVAL, "meta_step: task %d has %d support classes but %d query classes", t, cs.tab[t * 3 + 1], cq.tab[t * 3 + 1]);
    const int Ct = cs.Ct, ns = cs.n, nq = cq.n;
    MetaPlan p;
    int64_t cut = 0, shift = 0;
    const gm_model_t mp = internal_model(m, spt, &cut, &shift);
    gm_layout Lu;                                          // the caller's parameter layout (theta, out)
    GM_TRY(gm_make_layout(m, &Lu));
    GM_TRY(meta_plan(p, spt, qry, &mp, hp, ws, ws_bytes, Ct, ns, nq, nullptr));
    const gm_layout& L = p.L; const int T = p.T, C = L.n_out, K1 = K + 1; const int64_t Pp = p.Pp;
    p.uni_s = cs.uniform ? 1 : 0; p.uni_q = cq.uniform ? 1 : 0;
    p.qmax_s = cs.qmax; p.qmax_q = cq.qmax;
    GM_REQUIRE((int64_t)cs.rows.size() <= p.cap_s && (int64_t)cq.rows.size() <= p.cap_q, GM_EINVAL, "meta_step: class tables outgrew the workspace plan");
    p.S.pd = p.Q.pd = p.Q2.pd = p.pd.base ? &p.pd : nullptr;
    GM_TRY(pad_theta(p, &theta, Lu.P, cut, shift, st));
    // class tables -> pinned staging -> ONE asynchronous copy (no host synchronisation in the meta-step)
    const size_t n_rows = (size_t)(p.cap_s + p.cap_q), n_tab = n_rows + 8 * (size_t)T;
    GM_TRY(stage_to_device(p.rows_s, 4 * n_tab, st, [&](void* h) {
        int32_t* hp32 = (int32_t*)h;
        memset(hp32, 0, 4 * n_tab);
        memcpy(hp32, cs.rows.data(), 4 * cs.rows.size());
        memcpy(hp32 + p.cap_s, cq.rows.data(), 4 * cq.rows.size());
        memcpy(hp32 + n_rows, cs.tab.data(), 4 * cs.tab.size());
        memcpy(hp32 + n_rows + 3 * (size_t)T, cq.tab.data(), 4 * cq.tab.size());
        if (p.bound_ws) {
            // two-piece kernels: the layer-1 operand of task t is bounded by the largest feature of the graphs its subgraphs come from.  A step
            // that touches a LOOSE table (gm_store::h_feat_mean: largest entry more than 2^14 above the typical one, or not finite) runs
            // entirely on the three-piece kernels
            const gm_store* sto = spt->store;
            bool loose = false;
            int k = 0;
            for (const gm_batch* bb : {spt, qry}) {
                float* fb = reinterpret_cast<float*>(hp32 + n_rows + 6 * (size_t)T) + (size_t)(k++) * T;
                for (int t = 0; t < T; ++t) {
                    float mx = 0.f;
                    for (int sg = bb->h_set_sub_off[t]; sg < bb->h_set_sub_off[t + 1]; ++sg) {
                        const int gi = bb->h_graph[sg];
                        const float a = sto->h_feat_amax[gi], mean = sto->h_feat_mean[gi];
                        if (!(a <= 1.125899906842624e15f) || a > 16384.f * mean) loose = true;          // (2^50; 2^14 above the typical entry)
                        mx = a > mx ? a : mx;
                    }
                    fb[t] = mx;
                }
            }
            if (loose) {
                p.S.np = p.Q.np = p.Q2.np = 3; p.S.am = p.Q.am = p.Q2.am = nullptr; p.S.am_passes = p.Q.am_passes = p.Q2.am_passes = 0;
                p.pd.wam = nullptr; p.pd.viol = nullptr; p.viol = nullptr; p.bound_ws = nullptr;
            } else { p.S.feat_bound = p.featb_s; p.Q.feat_bound = p.Q2.feat_bound = p.featb_q; }
        }
    }));
    if (p.bound_ws) {
        GM_TRY(gm_batch_gains(spt, st)); GM_TRY(gm_batch_gains(qry, st));      // (computed once per batch, at its first two-piece step)
        // bound slots of this step: zero (the producers use atomicMax), then the maxima of theta's weight matrices (slot k = 0)
        GM_HIP(hipMemsetAsync(p.bound_ws, 0, sizeof(unsigned) * p.bound_words, st));
        p.pd.theta = theta;
        int64_t off[GM_MAX_GCN], n[GM_MAX_GCN];
        for (int l = 0; l < L.n_gcn; ++l) { off[l] = L.w_off[l]; n[l] = (int64_t)L.dims[l] * L.dims[l + 1]; }
        GM_TRY(gm_amax_segs(theta, off, n, L.n_gcn, p.pd.wam, GM_BOUND_PAD, st));
    }
    gm_prof_reset(GM_PROF_STEP_CATS);
    gm_prof_reset_cat(GM_PROF_GEMM_SPLIT_BYTES); gm_prof_reset_cat(GM_PROF_AGG_BOUND);
    gm_prof_reset_cat(GM_PROF_GEMM_BYTES); gm_prof_reset_cat(GM_PROF_WGRAD_BYTES); gm_prof_reset_cat(GM_PROF_HEAD);
    if (L.readout == GM_READOUT_MEAN) {      // the chunk tables of both batches, on st ahead of the event every stream of the step waits for
        GM_TRY(readout_tables(spt, st)); GM_TRY(readout_tables(qry, st));
        gm_prof_reset_cat(GM_PROF_READOUT); gm_prof_reset_cat(GM_PROF_READOUT_BWD);
    }
    tm.lap("plan");
    // Two streams: `st` carries the support chain (the serial dependency through the fast weights: forward -> loss ->
    // backward -> SGD, K times), `sq` carries the K+1 query evaluations, each of which only needs fw_k and the
    // prototypes of step k-1.  The small latency-bound support kernels thus overlap the throughput-bound query work.
    MetaStreams& ms = meta_streams();
    GM_TRY(ms.ensure(2 * K + 10));
    hipStream_t sq = hp->serialize ? st : ms.side;
    const bool two_q = p.nq_ctx == 2 && !hp->serialize && ms.side2;
    hipStream_t sq2 = two_q ? ms.side2 : sq;
    if (two_q) GM_TRY(gm_batch_hub_alt(qry, st));          // private hub counters / partial rows for the second query stream
    int ev = 0;
    auto signal = [&](hipStream_t from) -> hipEvent_t { hipEvent_t e = ms.ev[ev++]; (void)hipEventRecord(e, from); return e; };
    auto wait = [&](hipStream_t who, hipEvent_t e) { (void)hipStreamWaitEvent(who, e, 0); };
    {
        hipEvent_t e_in = signal(st);                      // inputs (theta, class tables, batches) are ready
        wait(sq, e_in);
        if (two_q) wait(sq2, e_in);
    }
    // the zero blocks behind T_L (GM_DEAD_ROWS=2), once per step: the caller's workspace is not preserved between calls.  On st BEHIND e_in -- the query streams
    // start without them: the one query backward of the step follows a wait for an event st records later (e_fw), the support backwards run on st itself
    GM_TRY(t_zero_fill(p.S, st)); GM_TRY(t_zero_fill(p.Q, st));
    if (two_q) GM_TRY(t_zero_fill(p.Q2, st));

    auto protos = [&](int k) -> float* { return p.protos + (int64_t)k * p.proto_sz; };   // prototypes of support step k
    const int hoist = hp->hoist_z1, sparse = hp->sparse_bwd;
    // One query evaluation (meta.py:129-141,152-154): forward on sq, then head + proto_loss_qry (+ head backward when the
    // meta-gradient is wanted) once the prototypes / weights it needs are ready.
    // Evaluation j (j = 0: theta, j >= 1: fw_j) runs in query context j % 2 on that context's stream when two query streams are used.
    auto q_ctx = [&](int j) -> GcnCtx& { return (two_q && (j & 1)) ? p.Q2 : p.Q; };
    auto q_str = [&](int j) -> hipStream_t { return (two_q && (j & 1)) ? sq2 : sq; };
    auto q_log = [&](int j) -> float* { return (two_q && (j & 1)) ? p.logit_q2 : p.logit_q; };
    auto qry_fwd = [&](int j, const float* w, int64_t wstride, PassKind kind) -> int {
        GcnCtx& c = q_ctx(j);
        if (c.np == 2) c.am_pass = j - 1;                  // (gcn_forward advances it: evaluation j records its bounds in pass j, whichever context runs it)
        return gcn_forward(c, w, wstride, q_log(j), q_str(j), hoist, 1, kind);
    };
    auto qry_loss = [&](int j, const float* w, int64_t wstride, int col, int kproto, bool grad) -> int {
        ProtoK pk{q_log(j), C, p.rows_q, Ct, nq, 1, protos(kproto), nullptr, p.lq, p.aq, K1, col, grad ? p.dlog_q : nullptr, grad ? p.dprotos : nullptr, 0, p.tab_q, p.uni_q};
        return head_loss(q_ctx(j), w, wstride, q_log(j), pk, grad ? 1 : 0, p.gq, Pp, sparse, q_str(j), p.qmax_q != 0);
    };
    // ---- support step 0 (meta.py:122-126) on st ; query evaluations 0 and 1 (meta.py:129-141) on sq.  Host enqueue order matters at the
    // start of a step (the GPU is idle and a launch costs the host ~5 us): the first query forward needs nothing but theta and is the head
    // of the longer chain on small shards, so it goes out first -- behind the support step's ~17 launches it started ~110 us late.
    // (Where the support chain is the longer one -- small query batches: the FirstMM shape lost 2.5 % -- its launches keep the lead.)
    const bool query_first = qry->rows >= 100000;
    if (query_first) GM_TRY(qry_fwd(0, theta, 0, PASS_FWD_ONLY));
    GM_TRY(support_head(p, hp, 0, theta, 0, p.fw_k(1), protos(0), st));
    hipEvent_t e_proto0 = signal(st);
    if (!query_first) GM_TRY(qry_fwd(0, theta, 0, PASS_FWD_ONLY));
    wait(q_str(0), e_proto0);
    GM_TRY(qry_loss(0, theta, 0, 0, 0, false));
    GM_TRY(support_bwd(p, hp, theta, 0, st));
    hipEvent_t e_fw = signal(st);                          // fw_1 ready (and, being later on st, the prototypes of step 0)
    wait(q_str(1), e_fw);
    GM_TRY(qry_fwd(1, p.fw_k(1), Pp, PASS_FWD_ONLY));
    GM_TRY(qry_loss(1, p.fw_k(1), Pp, 1, 0, false));
    bool have_grad = false;
    for (int k = 1; k < K; ++k) {            // meta.py:143-157
        GM_TRY(support_head(p, hp, k, p.fw_k(k), Pp, p.fw_k(k + 1), protos(k), st));
        GM_TRY(support_bwd(p, hp, p.fw_k(k), Pp, st));
        e_fw = signal(st);                                 // fw_{k+1} and the prototypes of step k are ready
        const int j = k + 1;
        wait(q_str(j), e_fw);
        const bool last = hp->need_meta_grad && k == K - 1;
        GM_TRY(qry_fwd(j, p.fw_k(k + 1), Pp, !last ? PASS_FWD_ONLY : (sparse && sparse_bwd_ok(p.L)) ? PASS_PLAIN : PASS_DIFF));       // only the last evaluation is differentiated
        GM_TRY(qry_loss(j, p.fw_k(k + 1), Pp, k + 1, k, last));
        if (last) {
            // first-order meta-gradient (no create_graph anywhere, meta.py:125,149): d L_q / d fw_K through the
            // query forward (on its query stream) plus d L_q / d fw_{K-1} through the prototypes of the last support forward (on st).
            hipEvent_t e_dp = signal(q_str(j));            // dprotos ready
            GM_TRY(gcn_backward(q_ctx(j), p.fw_k(k + 1), Pp, p.dlog_q, p.gq, Pp, q_str(j), sparse, 1));
            wait(st, e_dp);
            GM_HIP(hipMemsetAsync(p.dlog_s, 0, sizeof(float) * spt->subs * C, st));
            if (p.qmax_s) hipLaunchKernelGGL(k_protos_to_dlogits_ragged, dim3(T), dim3(256), 0, st, p.dprotos, p.rows_s, p.tab_s, Ct, C, p.dlog_s);
            else hipLaunchKernelGGL(k_protos_to_dlogits, dim3(T), dim3(256), 0, st, p.dprotos, p.rows_s, p.tab_s, Ct, C, p.dlog_s);
            GM_TRY(gcn_backward(p.S, p.fw_k(k), Pp, p.dlog_s, p.gp, Pp, st, sparse));
            have_grad = true;
        }
    }
    wait(st, signal(sq));                                  // join
    if (two_q) wait(st, signal(sq2));
    const int64_t tot = Lu.P + 2 * K1 + 1 + (int64_t)T * K1;
    hipLaunchKernelGGL(k_finalize, dim3((int)std::min<int64_t>(1024, (tot + 255) / 256)), dim3(256), 0, st,
                       have_grad ? p.gq : nullptr, p.gp, Pp, Lu.P, T, p.lq, p.aq, K1, out, cut, shift, p.viol);
    GM_HIP(hipGetLastError());
    gm_batch_mark_use(spt, st); gm_batch_mark_use(qry, st);
    return GM_OK;
}

// ================================================================================ adaptation and prediction (beyond the reference)
// gm_meta_adapt is the support chain of gm_meta_step alone (support_head / support_bwd on a SupportPlan of its own: forward -> k_head_loss -> backward with
// the fused SGD, K times); gm_proto_predict is one query forward at per-set parameters followed by k_head_predict.  Both use the three-piece split
// kernels (no bound slots).
static int adapt_plan(SupportPlan& p, const gm_batch* spt, const gm_model_t* m, const gm_hparams_t* hp, void* ws, int64_t ws_bytes, int64_t* need) {
    GM_TRY(support_prologue(p, spt, m, hp));
    Carver cv(ws, ws_bytes);
    const int C = p.L.n_out, K1 = p.K + 1;
    p.theta_p = cv.take<float>(p.Pp);
    p.fw = cv.take<float>(p.TP * p.K); p.g = cv.take<float>(p.TP);
    p.logit_s = cv.take<float>((int64_t)spt->subs * C); p.dlog_s = cv.take<float>((int64_t)spt->subs * C);
    p.protos = cv.take<float>(p.proto_sz);                      // every step overwrites them: the last support step's are the result
    p.ls = cv.take<float>((int64_t)p.T * K1); p.as_ = cv.take<float>((int64_t)p.T * K1);
    p.cap_s = spt->subs + (g_ragged ? (int64_t)spt->subs + p.T : 0);
    p.rows_s = cv.take<int32_t>(p.cap_s + 3 * (int64_t)p.T);      // one block [rows_s (cap_s) | tab_s (3T)]
    p.tab_s = p.rows_s ? p.rows_s + p.cap_s : nullptr;
    gcn_carve(p.S, cv);
    plan_planes(p.pd, p.L, p.T, p.K, p.fw, p.TP, !p.S.cone, cv);
    if (need) *need = cv.used + 256;
    GM_REQUIRE(cv.ok(), GM_ENOMEM, "meta_adapt: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)cv.used);
    return GM_OK;
}

extern "C" int64_t gm_adapt_ws_bytes(const gm_batch_t* spt, const gm_model_t* m, const gm_hparams_t* hp) {
    if (!spt || !m || !hp || hp->update_step < 0) return -1;
    SupportPlan p; int64_t need = 0, cut, shift;
    const gm_model_t mp = internal_model(m, spt, &cut, &shift);
    if (adapt_plan(p, spt, &mp, hp, nullptr, 0, &need) != GM_OK) return -1;
    return need;
}

extern "C" int gm_meta_adapt(const gm_batch_t* spt, const int32_t* y_spt, const gm_model_t* m, const gm_hparams_t* hp, const float* theta, float* fw_out,
                             int64_t fw_stride, float* protos_out, int32_t c_task, void* ws, int64_t ws_bytes, void* stream) {
    GM_REQUIRE(spt && y_spt && m && hp && theta && fw_out && protos_out && ws, GM_EINVAL, "meta_adapt: NULL argument");
    const int K = hp->update_step;
    GM_REQUIRE(K >= 0, GM_EINVAL, "meta_adapt: update_step must be >= 0 (got %d)", K);
    GM_REQUIRE(!hp->need_meta_grad, GM_EINVAL, "meta_adapt: need_meta_grad must be 0 (adaptation computes no meta-gradient)");
    GM_REQUIRE(hp->k_spt >= 1, GM_EINVAL, "meta_adapt: k_spt must be >= 1");
    GM_REQUIRE(((uintptr_t)theta & 15) == 0, GM_EINVAL, "meta_adapt: theta must be 16-byte aligned");
    gm_layout Lu;                                          // the caller's parameter layout (theta, fw_out)
    GM_TRY(gm_make_layout(m, &Lu));
    GM_REQUIRE(fw_stride >= Lu.P, GM_EINVAL, "meta_adapt: fw_stride %lld < P=%lld", (long long)fw_stride, (long long)Lu.P);
    hipStream_t st = (hipStream_t)stream;
    ClassTables cs;
    GM_TRY(class_tables(spt, y_spt, hp->k_spt, cs));
    GM_REQUIRE(c_task >= cs.Ct, GM_EINVAL, "meta_adapt: c_task=%d but a support set has %d classes", c_task, cs.Ct);
    SupportPlan p;
    int64_t cut = 0, shift = 0;
    const gm_model_t mp = internal_model(m, spt, &cut, &shift);
    GM_TRY(adapt_plan(p, spt, &mp, hp, ws, ws_bytes, nullptr));
    const int T = p.T, C = p.L.n_out; const int64_t Pp = p.Pp;
    p.Ct = cs.Ct; p.ns = cs.n; p.uni_s = cs.uniform ? 1 : 0; p.qmax_s = cs.qmax;
    p.S.pd = p.pd.base ? &p.pd : nullptr;
    GM_TRY(pad_theta(p, &theta, Lu.P, cut, shift, st));
    GM_TRY(t_zero_fill(p.S, st));      // the zero block behind T_L (GM_DEAD_ROWS=2), once per call
    // support class tables -> pinned staging -> one asynchronous copy
    const size_t n_tab = (size_t)p.cap_s + 3 * (size_t)T;
    GM_TRY(stage_to_device(p.rows_s, 4 * n_tab, st, [&](void* h) {
        int32_t* hp32 = (int32_t*)h;
        memset(hp32, 0, 4 * n_tab);
        memcpy(hp32, cs.rows.data(), 4 * cs.rows.size());
        memcpy(hp32 + p.cap_s, cs.tab.data(), 4 * cs.tab.size());
    }));
    // gm_meta_step's support chain (meta.py:122-126,145-151); K = 0: the forward and the prototypes only
    for (int k = 0; k < std::max(K, 1); ++k) {
        const float* w = k ? p.fw_k(k) : theta;
        const int64_t wstride = k ? Pp : 0;
        GM_TRY(support_head(p, hp, k, w, wstride, K > 0 ? p.fw_k(k + 1) : nullptr, p.protos, st));
        if (K > 0) GM_TRY(support_bwd(p, hp, w, wstride, st));
    }
    const int64_t big = std::max<int64_t>(Lu.P, (int64_t)c_task * C);
    hipLaunchKernelGGL(k_adapt_out, dim3((int)std::min<int64_t>(256, (big + 255) / 256), T), dim3(256), 0, st, K ? p.fw_k(K) : theta, K ? Pp : 0, Lu.P, cut, shift,
                       fw_out, fw_stride, p.protos, p.Ct, p.tab_s, c_task, C, protos_out);
    GM_HIP(hipGetLastError());
    gm_batch_mark_use(spt, st);
    return GM_OK;
}

struct PredictPlan {
    gm_layout L; int64_t Pp;
    GcnCtx Q;
    float *params_p, *logits;
    int32_t* n_cls;
};

static int predict_plan(PredictPlan& p, const gm_batch* qry, const gm_model_t* m, const gm_hparams_t* hp, bool own_logits, void* ws, int64_t ws_bytes, int64_t* need) {
    GM_TRY(plan_prologue(m, hp, qry, p.L, p.Pp, p.Q));
    Carver cv(ws, ws_bytes);
    p.params_p = cv.take<float>((int64_t)qry->sets * p.Pp);
    p.logits = own_logits ? cv.take<float>((int64_t)qry->subs * p.L.n_out) : nullptr;
    p.n_cls = cv.take<int32_t>(qry->sets);
    gcn_carve(p.Q, cv);
    if (need) *need = cv.used + 256;
    GM_REQUIRE(cv.ok(), GM_ENOMEM, "proto_predict: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)cv.used);
    return GM_OK;
}

extern "C" int64_t gm_predict_ws_bytes(const gm_batch_t* qry, const gm_model_t* m, const gm_hparams_t* hp) {
    if (!qry || !m || !hp) return -1;
    PredictPlan p; int64_t need = 0, cut, shift;
    const gm_model_t mp = internal_model(m, qry, &cut, &shift);
    if (predict_plan(p, qry, &mp, hp, true, nullptr, 0, &need) != GM_OK) return -1;
    return need;
}

extern "C" int gm_proto_predict(const gm_batch_t* qry, const gm_model_t* m, const gm_hparams_t* hp, const float* params, int64_t param_stride,
                                const float* protos, const int32_t* n_classes, int32_t c_task, float* logits_out, float* logp_out, int32_t* pred_out,
                                void* ws, int64_t ws_bytes, void* stream) {
    GM_REQUIRE(qry && m && hp && params && protos && n_classes && logp_out && pred_out && ws, GM_EINVAL, "proto_predict: NULL argument");
    gm_layout Lu;
    GM_TRY(gm_make_layout(m, &Lu));
    GM_REQUIRE(param_stride >= Lu.P, GM_EINVAL, "proto_predict: param_stride %lld < P=%lld", (long long)param_stride, (long long)Lu.P);
    GM_REQUIRE(c_task >= 1 && c_task <= 256, GM_EINVAL, "proto_predict: c_task=%d outside [1, 256]", c_task);
    for (int t = 0; t < qry->sets; ++t)
        GM_REQUIRE(n_classes[t] >= 1 && n_classes[t] <= c_task, GM_EINVAL, "proto_predict: set %d has %d classes, outside [1, c_task=%d]", t, n_classes[t], c_task);
    const size_t lds = sizeof(float) * 4 * (size_t)c_task * (Lu.n_out + 1);
    GM_REQUIRE(lds <= 160 * 1024, GM_ERANGE, "proto_predict: %d classes x %d logits per set is outside the scoring kernel's range", c_task, Lu.n_out);
    hipStream_t st = (hipStream_t)stream;
    PredictPlan p;
    int64_t cut = 0, shift = 0;
    const gm_model_t mp = internal_model(m, qry, &cut, &shift);
    GM_TRY(predict_plan(p, qry, &mp, hp, logits_out == nullptr, ws, ws_bytes, nullptr));
    const int T = qry->sets;
    float* logits = logits_out ? logits_out : p.logits;
    if (T > 0) {
        hipLaunchKernelGGL(k_pad_params_sets, dim3((int)std::min<int64_t>(256, (p.L.P + 255) / 256), T), dim3(256), 0, st, params, param_stride, Lu.P, cut, shift,
                           p.params_p, p.Pp);
        GM_HIP(hipGetLastError());
        GM_TRY(stage_to_device(p.n_cls, 4 * (size_t)T, st, [&](void* h) { memcpy(h, n_classes, 4 * (size_t)T); }));
    }
    if (qry->subs > 0) {
        // gm_meta_step's query evaluation nobody differentiates (PASS_FWD_ONLY: the fused aggregate + GEMM where eligible), then the scoring kernel
        GM_TRY(gcn_forward(p.Q, p.params_p, p.Pp, logits, st, hp->hoist_z1, 1, PASS_FWD_ONLY));
        HeadK hk = make_head(p.Q, p.params_p, p.Pp);
        if (lds > 64 * 1024) GM_TRY(gm_func_full_lds((const void*)k_head_predict));
        hipLaunchKernelGGL(k_head_predict, dim3((qry->subs + 3) / 4), dim3(256), lds, st, hk, protos, (int)c_task, p.n_cls, logits, logp_out, pred_out);
        GM_HIP(hipGetLastError());
    }
    gm_batch_mark_use(qry, st);
    return GM_OK;
}

// ================================================================================ after the all-reduce
// grad[i] = head[i] / task count ;  found_inf = isnan(losses_q[K] / task count)  (meta.py:161-163).  `head` is the
// (all-reduced) [grad(P) | losses_q(K1) | corrects(K1) | count] block of gm_meta_step's output.
__global__ void k_meta_finish(const float* head, int64_t P, int K1, float* grad, float* found_inf) {
    const float cnt = head[P + 2 * K1];
    for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < P; id += (int64_t)gridDim.x * blockDim.x) grad[id] = head[id] / cnt;
    if (blockIdx.x == 0 && threadIdx.x == 0) { const float l = head[P + K1 - 1] / cnt; *found_inf = (l != l) ? 1.f : 0.f; }
}

extern "C" int gm_meta_finish(const float* head, int64_t P, int32_t K1, float* grad, float* found_inf, void* stream) {
    GM_REQUIRE(head && grad && found_inf && P >= 1 && K1 >= 1, GM_EINVAL, "meta_finish: bad arguments");
    hipLaunchKernelGGL(k_meta_finish, dim3((int)std::min<int64_t>(512, (P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, head, P, K1, grad, found_inf);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// The same guard AND the Adam step (meta.py:97,161-169: optim.Adam(lr = meta_lr), default betas / eps, no weight decay) in ONE launch: between two
// meta-steps the stream otherwise carries k_meta_finish + three launches of torch's fused optimiser, and the host spends ~100 us inside
// optimizer.step() -- on the small configurations (1.5 - 4 ms per meta-step) that is where the GPU sat empty.  torch's fused Adam rule, in fp32:
//   m <- m + (1 - b1) (g - m);  v <- b2 v + (1 - b2) g g;  theta <- theta - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with t = step + 1; a NaN reduced query loss leaves theta, m, v and the step count untouched (`if torch.isnan(loss_q): pass`).  steps[0 .. n_steps)
// are the per-parameter step counters of the torch optimiser's state (all equal): read by every block, written by the LAST block to finish
// (ticket), so that no block can see the incremented value.
__global__ __launch_bounds__(256) void k_meta_finish_adam(const float* head, int64_t P, int K1, float* theta, float* m, float* v, float* grad, float* steps, int n_steps,
                                                          float lr, float b1, float b2, float eps, float* found_inf, unsigned* ticket) {
    const float cnt = head[P + 2 * K1];
    const float l = head[P + K1 - 1] / cnt;
    const bool skip = l != l;
    const float t = steps[0] + 1.f;
    const float bc1 = (float)(1.0 - pow((double)b1, (double)t)), bc2s = sqrtf((float)(1.0 - pow((double)b2, (double)t)));
    const float step_size = lr / bc1;
    for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < P; id += (int64_t)gridDim.x * blockDim.x) {
        const float g = head[id] / cnt;
        grad[id] = g;
        if (skip) continue;
        const float m0 = m[id], v0 = v[id];
        const float m1 = m0 + (1.f - b1) * (g - m0);
        const float v1 = b2 * v0 + (1.f - b2) * g * g;
        m[id] = m1; v[id] = v1;
        theta[id] -= step_size * (m1 / (sqrtf(v1) / bc2s + eps));
    }
    __syncthreads();                                       // every thread of this block has read steps[0]
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {      // every block has
            *ticket = 0u;
            *found_inf = skip ? 1.f : 0.f;
            if (!skip) for (int i = 0; i < n_steps; ++i) steps[i] = t;
        }
    }
}

extern "C" int gm_meta_finish_adam(const float* head, int64_t P, int32_t K1, float* theta, float* exp_avg, float* exp_avg_sq, float* grad, float* steps, int32_t n_steps,
                                   float lr, float beta1, float beta2, float eps, float* found_inf, uint32_t* ticket, void* stream) {
    GM_REQUIRE(head && theta && exp_avg && exp_avg_sq && grad && steps && found_inf && ticket && P >= 1 && K1 >= 1 && n_steps >= 1, GM_EINVAL, "meta_finish_adam: bad arguments");
    hipLaunchKernelGGL(k_meta_finish_adam, dim3((int)std::min<int64_t>(256, (P + 511) / 512)), dim3(256), 0, (hipStream_t)stream, head, P, (int)K1, theta, exp_avg, exp_avg_sq, grad,
                       steps, (int)n_steps, lr, beta1, beta2, eps, found_inf, ticket);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// ================================================================================ mean readout (gm_set_readout(GM_READOUT_MEAN), include/gmeta_hip.h)
// P[s, :] = (sum over the rows of subgraph s of H_L[r, :]) / n_s and its backward dQ_L[r, :] = H_L[r, :] > 0 ? G[s, :] / n_s : 0.  Subgraphs run from one row
// to over a thousand, so the unit of work is a CHUNK of up to GM_RO_ROWS consecutive rows of one subgraph (host table, built once per batch from its
// sub_off mirror): one workgroup per chunk.  The summation order is fixed by n_s and Hd alone: inside a chunk, row slot j (of RS = 256 / min(Hd / V, 256))
// adds rows j, j + RS, ... in ascending order, the slots are added in ascending order; a subgraph of one chunk is divided and stored right there, the
// chunks of a larger one go to `part` and are added in ascending order by k_readout_mean_fin.  No atomics.
// Defined HERE, behind every kernel a call without the mode launches: those keep their place in the code object (see the ragged-task kernels above).
#define GM_RO_ROWS 64
#define GM_RO_NT 256
template <int V> struct RoVec;
template <> struct RoVec<1> {
    float v;
    __device__ __forceinline__ static RoVec zero() { return RoVec{0.f}; }
    __device__ __forceinline__ static RoVec load(const float* p) { return RoVec{*p}; }
    __device__ __forceinline__ void store(float* p) const { *p = v; }
    __device__ __forceinline__ void add(const RoVec& o) { v += o.v; }
    __device__ __forceinline__ void div(float d) { v /= d; }
    __device__ __forceinline__ RoVec where_pos(const RoVec& g) const { return RoVec{v > 0.f ? g.v : 0.f}; }
};
template <> struct RoVec<4> {
    float4 v;
    __device__ __forceinline__ static RoVec zero() { return RoVec{make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ __forceinline__ static RoVec load(const float* p) { return RoVec{*reinterpret_cast<const float4*>(p)}; }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
    __device__ __forceinline__ void add(const RoVec& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
    __device__ __forceinline__ void div(float d) { v.x /= d; v.y /= d; v.z /= d; v.w /= d; }
    __device__ __forceinline__ RoVec where_pos(const RoVec& g) const {
        return RoVec{make_float4(v.x > 0.f ? g.v.x : 0.f, v.y > 0.f ? g.v.y : 0.f, v.z > 0.f ? g.v.z : 0.f, v.w > 0.f ? g.v.w : 0.f)};
    }
};

// V = 4: 16-byte loads / stores (Hd % 4 == 0, 16-byte aligned bases); V = 1: the scalar path.  chunks[k] = {row0, rows, subgraph, rows of the subgraph}
template <int V>
__global__ __launch_bounds__(GM_RO_NT) void k_readout_mean(const float* __restrict__ H, int Hd, const int4* __restrict__ chunks, float* __restrict__ P,
                                                           float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[GM_RO_NT * V];
    typedef RoVec<V> Vec;
    const int4 ch = chunks[blockIdx.x];
    const int nr = ch.y, ns = ch.w;
    const int nv = Hd / V, cpp = min(nv, GM_RO_NT), RS = GM_RO_NT / cpp;      // column vectors per row; of them per pass; row slots
    const int tid = threadIdx.x, slot = tid / cpp, cl = tid - slot * cpp;
    const bool single = ns <= GM_RO_ROWS;
    float* out = single ? P + (int64_t)ch.z * Hd : part + (int64_t)blockIdx.x * Hd;
    const float* base = H + (int64_t)ch.x * Hd;
    for (int c0 = 0; c0 < nv; c0 += cpp) {
        const int c = c0 + cl;
        Vec acc = Vec::zero();
        if (slot < RS && c < nv) {
            const float* p = base + c * V;
            int r = slot;
            for (; r + 3 * RS < nr; r += 4 * RS) {      // four loads in flight, added in row order
                const Vec a0 = Vec::load(p + (int64_t)r * Hd), a1 = Vec::load(p + (int64_t)(r + RS) * Hd), a2 = Vec::load(p + (int64_t)(r + 2 * RS) * Hd),
                          a3 = Vec::load(p + (int64_t)(r + 3 * RS) * Hd);
                acc.add(a0); acc.add(a1); acc.add(a2); acc.add(a3);
            }
            for (; r < nr; r += RS) acc.add(Vec::load(p + (int64_t)r * Hd));
        }
        acc.store(sm + tid * V);
        __syncthreads();
        if (slot == 0 && c < nv) {
            Vec t = Vec::load(sm + cl * V);
            for (int j = 1; j < RS; ++j) t.add(Vec::load(sm + (j * cpp + cl) * V));
            if (single) t.div((float)ns);
            t.store(out + c * V);
        }
        __syncthreads();
    }
}
// multi[m] = {subgraph, first chunk, chunks, rows}: the partials of a subgraph of more than one chunk, in chunk order
__global__ __launch_bounds__(GM_RO_NT) void k_readout_mean_fin(const float* __restrict__ part, int Hd, const int4* __restrict__ multi, float* __restrict__ P) {
    const int4 m = multi[blockIdx.x];
    const float* p = part + (int64_t)m.y * Hd;
    for (int col = threadIdx.x; col < Hd; col += GM_RO_NT) {
        float t = p[col];
        for (int k = 1; k < m.z; ++k) t += p[(int64_t)k * Hd + col];
        P[(int64_t)m.x * Hd + col] = t / (float)m.w;
    }
}
// Every row of dQ is written (nothing zero-fills it first)
template <int V>
__global__ __launch_bounds__(GM_RO_NT) void k_readout_mean_bwd(const float* __restrict__ H, const float* __restrict__ G, int Hd, const int4* __restrict__ chunks,
                                                               float* __restrict__ dQ) {
    typedef RoVec<V> Vec;
    const int4 ch = chunks[blockIdx.x];
    const int nr = ch.y;
    const int nv = Hd / V, cpp = min(nv, GM_RO_NT), RS = GM_RO_NT / cpp;
    const int tid = threadIdx.x, slot = tid / cpp, cl = tid - slot * cpp;
    if (slot >= RS) return;
    for (int c = cl; c < nv; c += cpp) {
        Vec g = Vec::load(G + (int64_t)ch.z * Hd + c * V);
        g.div((float)ch.w);
        const int64_t off = (int64_t)ch.x * Hd + c * V;
        int r = slot;
        for (; r + 3 * RS < nr; r += 4 * RS) {
            const Vec a0 = Vec::load(H + off + (int64_t)r * Hd), a1 = Vec::load(H + off + (int64_t)(r + RS) * Hd), a2 = Vec::load(H + off + (int64_t)(r + 2 * RS) * Hd),
                      a3 = Vec::load(H + off + (int64_t)(r + 3 * RS) * Hd);
            a0.where_pos(g).store(dQ + off + (int64_t)r * Hd); a1.where_pos(g).store(dQ + off + (int64_t)(r + RS) * Hd);
            a2.where_pos(g).store(dQ + off + (int64_t)(r + 2 * RS) * Hd); a3.where_pos(g).store(dQ + off + (int64_t)(r + 3 * RS) * Hd);
        }
        for (; r < nr; r += RS) Vec::load(H + off + (int64_t)r * Hd).where_pos(g).store(dQ + off + (int64_t)r * Hd);
    }
}

static int64_t readout_chunk_count(const gm_batch* b) {
    int64_t n = 0;
    for (int s = 0; s < b->subs; ++s) n += (b->h_sub_off[s + 1] - b->h_sub_off[s] + GM_RO_ROWS - 1) / GM_RO_ROWS;
    return n;
}
// The chunk tables of a batch, built at its first call under the mode (on s, ordered behind the batch's build) and kept in its slabs, like gm_batch_gains
static int readout_tables(const gm_batch* cb, hipStream_t s) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    gm_batch* b = const_cast<gm_batch*>(cb);
    if (b->d_ro_chunks) {
        // built by an earlier call: a caller on another stream is ordered behind that call's upload (no event: the upload was synchronised)
        if (s != b->ro_stream && b->ro_ev) GM_HIP(hipStreamWaitEvent(s, b->ro_ev, 0));
        return GM_OK;
    }
    std::vector<int32_t> tab, multi;
    for (int sg = 0; sg < b->subs; ++sg) {
        const int r0 = b->h_sub_off[sg], ns = b->h_sub_off[sg + 1] - r0, first = (int)(tab.size() / 4);
        GM_REQUIRE(ns >= 1, GM_EINVAL, "mean readout: subgraph %d has no rows", sg);
        for (int r = 0; r < ns; r += GM_RO_ROWS) { const int32_t e[4] = {r0 + r, std::min(GM_RO_ROWS, ns - r), sg, ns}; tab.insert(tab.end(), e, e + 4); }
        if (ns > GM_RO_ROWS) { const int32_t e[4] = {sg, first, (int)(tab.size() / 4) - first, ns}; multi.insert(multi.end(), e, e + 4); }
    }
    const int32_t n_chunks = (int32_t)(tab.size() / 4), n_multi = (int32_t)(multi.size() / 4);
    tab.insert(tab.end(), multi.begin(), multi.end());
    int32_t* d = nullptr;
    GM_TRY(gm_balloc(b, &d, tab.size() + 4, b->stream));                                   // (the batch's slabs: freed with it, on its own stream)
    GM_TRY(gm_batch_wait_build(b, s));
    { gm_stager stg(s); GM_TRY(stg.upload(d, tab)); }
    // later callers may come on other streams (two threads sharing the batch; the query streams of a step wait for st anyway): an event behind the upload
    // for them to wait on -- where none can be made, the upload is finished before anybody learns of the tables
    if (hipEventCreateWithFlags(&b->ro_ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(b->ro_ev, s) != hipSuccess) {
        (void)hipGetLastError();
        if (b->ro_ev) { (void)hipEventDestroy(b->ro_ev); b->ro_ev = nullptr; }
        GM_HIP(hipStreamSynchronize(s));
    }
    b->ro_stream = s;
    b->n_ro_chunks = n_chunks; b->n_ro_multi = n_multi; b->d_ro_multi = d + 4 * (size_t)n_chunks; b->d_ro_chunks = d;
    gm_batch_mark_use(b, s);
    return GM_OK;
}
static bool readout_vec_ok(const GcnCtx& c, const float* a, const float* b2, const float* c2) {
    return c.L.dims[c.L.n_gcn] % 4 == 0 && (((uintptr_t)a | (uintptr_t)b2 | (uintptr_t)c2) & 15) == 0;
}
static int readout_fwd(const GcnCtx& c, hipStream_t st) {
    const gm_batch* b = c.b; const int Hd = c.L.dims[c.L.n_gcn];
    if (b->n_ro_chunks == 0) return GM_OK;
    GM_REQUIRE(b->d_ro_chunks && c.Pool && c.ro_part, GM_EINVAL, "mean readout: the batch's chunk tables or the pooled buffers are missing");
    const float* H = c.H[c.L.n_gcn - 1];
    const int4* chunks = reinterpret_cast<const int4*>(b->d_ro_chunks);
    gm_prof_begin(GM_PROF_READOUT, st, 4 * (int64_t)b->rows * Hd + 4 * (int64_t)b->subs * Hd);
    if (readout_vec_ok(c, H, c.Pool, c.ro_part)) hipLaunchKernelGGL(k_readout_mean<4>, dim3(b->n_ro_chunks), dim3(GM_RO_NT), 0, st, H, Hd, chunks, c.Pool, c.ro_part);
    else hipLaunchKernelGGL(k_readout_mean<1>, dim3(b->n_ro_chunks), dim3(GM_RO_NT), 0, st, H, Hd, chunks, c.Pool, c.ro_part);
    if (b->n_ro_multi > 0)
        hipLaunchKernelGGL(k_readout_mean_fin, dim3(b->n_ro_multi), dim3(GM_RO_NT), 0, st, (const float*)c.ro_part, Hd, reinterpret_cast<const int4*>(b->d_ro_multi), c.Pool);
    gm_prof_end(GM_PROF_READOUT, st);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
// dQ_L (c.bufA, every row) from G (c.Gpool, written by the head's backward) and H_L
static int readout_bwd(const GcnCtx& c, hipStream_t st) {
    const gm_batch* b = c.b; const int Hd = c.L.dims[c.L.n_gcn];
    if (b->n_ro_chunks == 0) return GM_OK;
    GM_REQUIRE(b->d_ro_chunks && c.Gpool, GM_EINVAL, "mean readout: the batch's chunk tables or the pooled buffers are missing");
    const float* H = c.H[c.L.n_gcn - 1];
    const int4* chunks = reinterpret_cast<const int4*>(b->d_ro_chunks);
    gm_prof_begin(GM_PROF_READOUT_BWD, st, 8 * (int64_t)b->rows * Hd + 4 * (int64_t)b->subs * Hd);
    if (readout_vec_ok(c, H, c.Gpool, c.bufA)) hipLaunchKernelGGL(k_readout_mean_bwd<4>, dim3(b->n_ro_chunks), dim3(GM_RO_NT), 0, st, H, (const float*)c.Gpool, Hd, chunks, c.bufA);
    else hipLaunchKernelGGL(k_readout_mean_bwd<1>, dim3(b->n_ro_chunks), dim3(GM_RO_NT), 0, st, H, (const float*)c.Gpool, Hd, chunks, c.bufA);
    gm_prof_end(GM_PROF_READOUT_BWD, st);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// ================================================================================ head + loss, exported for numerics tests
// One head-and-loss launch on the caller's own H, parameters, labels and prototypes (include/gmeta_hip.h).  path 0: k_head_loss through head_loss_launch, the
// code head_loss() runs; path 1: k_head_fwd, k_proto, k_head_bwd as gm_gcn_forward / gm_proto_loss_* / gm_gcn_backward issue them.  Host code only.
extern "C" int gm_dense_head_loss(const gm_batch_t* b, const float* H, int32_t Hd, int32_t nc, int32_t compact, int32_t C, const float* params,
                                  int64_t param_stride, int64_t wl_off, int64_t bl_off, const int32_t* centre_local, const int32_t* y, int32_t mode,
                                  int32_t n_support, const float* protos, int32_t c_task, const int32_t* spt_labels, const int32_t* spt_counts, float* logits,
                                  float* dlogits, float* dprotos, float* protos_out, float* loss, float* acc, int32_t bwd, float* dparams,
                                  int64_t dparam_stride, float* dQ, float* Gc, const float* sgd_cur, float* sgd_next, int64_t sgd_stride, float sgd_lr,
                                  uint32_t* dq_amax, int32_t path, int32_t* launched, void* stream) {
    GM_REQUIRE(b && H && params && y && logits && loss && acc, GM_EINVAL, "dense_head_loss: NULL argument");
    GM_REQUIRE(Hd >= 1 && Hd <= 2048 && C >= 1 && C <= 64 && (nc == 1 || nc == 2), GM_ERANGE, "dense_head_loss: Hd=%d C=%d nc=%d out of range", Hd, C, nc);
    GM_REQUIRE(path == 0 || path == 1, GM_EINVAL, "dense_head_loss: path is 0 (fused) or 1 (unfused)");
    GM_REQUIRE(compact ? (nc == b->centres || nc == 1) : nc == b->centres, GM_EINVAL, "dense_head_loss: nc=%d on a batch of %d centre(s) per subgraph", nc, b->centres);
    GM_REQUIRE(!compact || !centre_local, GM_EINVAL, "dense_head_loss: a compact H has no centre table to override");
    const int hc = nc * Hd;
    GM_REQUIRE(wl_off >= 0 && bl_off >= 0 && (bl_off >= wl_off + (int64_t)C * hc || wl_off >= bl_off + C), GM_EINVAL, "dense_head_loss: Wl and bl overlap");
    const int64_t p_end = std::max(wl_off + (int64_t)C * hc, bl_off + C);
    GM_REQUIRE(param_stride == 0 || param_stride >= p_end, GM_EINVAL, "dense_head_loss: param_stride %lld < %lld", (long long)param_stride, (long long)p_end);
    GM_REQUIRE(mode == 0 || mode == 1, GM_EINVAL, "dense_head_loss: mode is 0 (support) or 1 (query)");
    if (mode == 0) GM_REQUIRE(n_support >= 1 && !protos && !dprotos, GM_EINVAL, "dense_head_loss: mode 0 takes n_support >= 1 and neither protos nor dprotos");
    else GM_REQUIRE(protos && c_task >= 1 && !protos_out, GM_EINVAL, "dense_head_loss: mode 1 takes protos and c_task >= 1, and has no protos_out");
    GM_REQUIRE(!spt_labels == !spt_counts && (!spt_labels || (mode == 1 && g_ragged)), GM_EINVAL, "dense_head_loss: support classes go with mode 1 in ragged-task mode");
    GM_REQUIRE(!dprotos || dlogits, GM_EINVAL, "dense_head_loss: dprotos is written with dlogits");
    GM_REQUIRE(!(dQ && Gc), GM_EINVAL, "dense_head_loss: dQ together with Gc");
    if (bwd) GM_REQUIRE(dlogits && dparams && (dQ || Gc) && (b->sets == 1 || dparam_stride >= p_end), GM_EINVAL,
                        "dense_head_loss: the backward needs dlogits, dparams, one of dQ and Gc, and dparam_stride >= %lld", (long long)p_end);
    else GM_REQUIRE(!dQ && !Gc && !sgd_next && !dq_amax, GM_EINVAL, "dense_head_loss: dQ, Gc, the SGD step and dq_amax are outputs of the backward");
    GM_REQUIRE(!sgd_next || (sgd_cur && path == 0 && (b->sets == 1 || sgd_stride >= p_end)), GM_EINVAL, "dense_head_loss: the SGD step needs cur, the fused launch and a stride >= %lld", (long long)p_end);
    GM_REQUIRE(!dq_amax || dQ, GM_EINVAL, "dense_head_loss: dq_amax goes with dQ");
    hipStream_t st = (hipStream_t)stream;
    ClassTables ct, cs;
    if (spt_labels) {      // the support side's classes of every set (all class_tables_ragged reads of it)
        cs.tab.assign((size_t)b->sets * 3, 0);
        for (int t = 0; t < b->sets; ++t) {
            GM_REQUIRE(spt_counts[t] >= 1 && spt_counts[t] <= c_task, GM_EINVAL, "dense_head_loss: set %d has %d support classes, c_task = %d", t, spt_counts[t], c_task);
            cs.tab[t * 3 + 1] = spt_counts[t];
            cs.labels.insert(cs.labels.end(), spt_labels + cs.labels.size(), spt_labels + cs.labels.size() + spt_counts[t]);
        }
    }
    GM_TRY(class_tables(b, y, mode == 0 ? n_support : 0, ct, spt_labels ? &cs : nullptr));
    if (mode == 1) {      // as gm_proto_loss_qry
        for (int t = 0; t < b->sets; ++t)
            GM_REQUIRE(g_ragged ? ct.tab[t * 3 + 1] <= c_task : ct.tab[t * 3 + 1] == c_task, GM_EINVAL,
                       "dense_head_loss: set %d has %d query classes but the prototypes hold %d per set", t, ct.tab[t * 3 + 1], c_task);
        GM_REQUIRE(c_task <= 256 && (int64_t)c_task * ct.n <= 16384, GM_ERANGE, "dense_head_loss: c_task=%d with %d rows per class is outside the kernel's range", c_task, ct.n);
    }
    const int Ct = mode == 1 ? c_task : ct.Ct;
    const bool ragged = ct.qmax != 0;
    int32_t* d_rows = nullptr;
    GM_TRY(upload_tables(ct, &d_rows, st));
    HeadK hk{};
    hk.H = H; hk.ldh = Hd; hk.Hd = Hd;
    hk.sub_off = b->d_sub_off; hk.centre = centre_local ? centre_local : b->d_centre; hk.nc = nc; hk.sub_set = b->d_sub_set; hk.set_sub_off = b->d_set_sub_off;
    hk.params = params; hk.pstride = param_stride; hk.wl_off = wl_off; hk.bl_off = bl_off; hk.hc = hc; hk.C = C; hk.subs = b->subs; hk.compact = compact ? 1 : 0;
    hk.dq_amax = dq_amax; hk.subs_per_set = head_subs_per_set(b);
    int rc = GM_OK;
    if (path == 0) {
        const ProtoK pk{logits, C, d_rows, Ct, ct.n, mode, protos, protos_out, loss, acc, 1, 0, dlogits, dprotos, 0, d_rows + ct.rows.size(), (ct.uniform && ct.Ct == Ct) ? 1 : 0};
        rc = head_loss_launch(b, hk, logits, pk, bwd ? 1 : 0, dparams, dparam_stride, dQ, Gc, SgdK{sgd_cur, sgd_stride, sgd_next, sgd_stride, sgd_lr}, ragged, 1, launched, st);
    } else {
        hipLaunchKernelGGL(k_head_fwd, dim3((b->subs + 3) / 4), dim3(256), 0, st, hk, logits);
        if (dlogits && hipMemsetAsync(dlogits, 0, sizeof(float) * b->subs * C, st) != hipSuccess) { gm_set_error("dense_head_loss: memset failed"); rc = GM_EHIP; }
        if (rc == GM_OK) {
            const ProtoK pk{logits, C, d_rows, Ct, ct.n, mode, protos, protos_out, loss, acc, 1, 0, dlogits, dprotos, 0, d_rows + ct.rows.size()};
            rc = launch_proto(b, pk, ragged, st);
        }
        if (rc == GM_OK && bwd) hipLaunchKernelGGL(k_head_bwd, dim3(b->sets), dim3(256), 0, st, hk, (const float*)dlogits, dparams, dparam_stride, dQ, Gc);
        if (rc == GM_OK && hipGetLastError() != hipSuccess) { gm_set_error("dense_head_loss: launch failed"); rc = GM_EHIP; }
        if (launched) { launched[0] = 256; launched[1] = 0; launched[2] = ragged ? 1 : 0; }
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == GM_OK) { gm_set_error("dense_head_loss: kernel failed"); rc = GM_EHIP; }
    gm_dev_free(d_rows, st);
    gm_batch_mark_use(b, st);
    return rc;
}
