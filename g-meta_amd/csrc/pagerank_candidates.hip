// Top-k rooted-PageRank partners per source (gm_store_pagerank_candidates): the selection over one round's state of the walk while it is still in scratch, so
// that only [m, k] leaves the device.  The DEFINITION -- candidate set, score, ranking key, padding -- is in include/gmeta_hip.h;
// tests/pagerank_candidate_ref.py restates it.  The walk and the export are pair_pagerank.hip's (a third `emit` on ppr_rounds); this file is
// gm_pprc_round, what that emit runs on P[N, Br] = p of the round's Br columns (row-major, Br a multiple of 64):
//   exclusion   k_pprc_exclude: a wave per column stores +0.0f over P[w, c] for w in {a} + G(a) of the column's source a.  P is scratch; afterwards the
//               candidates of a column are exactly its positive entries.
//   select      P is read the way the walk reads it: lanes are columns, a wave streams a contiguous range of rows past in whole 256-byte pieces,
//               GM_PPRC_UNROLL reads in flight per lane.  A workgroup of eight waves takes a slab of 64 columns and eight consecutive row ranges.
//               k_pprc_hist counts eight bits of the score per pass from the top into a 256-bin x 64-column histogram in LDS (64 KiB: two workgroups
//               per CU; bin-major, so the 64 lanes of an add hit 64 different words) and adds its non-zero bins to the round's global histogram;
//               k_pprc_pick scans a column's 256 bins from the top, fixes the next digit of the k-th largest score and zeroes the bins for the next pass.
//               The first pass counts the positive entries: that is |R(a)|.  A column is done as soon as the chosen bin is wanted whole (or the whole
//               set is: total <= k); a slab whose columns are all done costs a later pass one load per lane.
//   ties        a column still open after the fourth pass has more entries AT the threshold score than it may keep: the ranking wants the lowest ids.
//               k_pprc_ties counts them per (row range, column), k_pprc_tie_scan turns the counts into exclusive prefixes over the ranges, and the
//               collect pass keeps a range's first (need - prefix) of them in row order.
//   collect     k_pprc_collect: the same sweep once more; every survivor's key goes to the column's list (at most 1,024 keys; the slot is an integer
//               atomic, the order of arrival is undone by the sort).
//   sort        k_pprc_out: a workgroup per OUTPUT row (duplicates of a source share its column) sorts the column's keys in LDS and writes the row
//               with the padding (gm_cand_sort_write, gm_internal.h: the code of gm_store_pair_candidates) and the total.
// Integer work throughout: no float arithmetic, no float atomics; integer atomics only on histogram counts and list slots, whose order cannot change the
// result.  No scratch memory in the kernels.  Everything runs on the caller's stream.
#include "gm_nbr.h"

#define GM_PPRC_THREADS 512               // the sweeps: eight waves, one row range each
#define GM_PPRC_WAVES (GM_PPRC_THREADS / GM_WAVE)
#define GM_PPRC_UNROLL 8                  // row reads of P in flight per lane
#define GM_PPRC_MIN_ROWS 16               // rows per range at least (small graphs: fewer ranges)
#define GM_PPRC_BINS 256

// a column of the select: the digits of the threshold score fixed so far (prefix under mask), how many entries AT them are still wanted, and whether the
// column is closed: every entry with (bits & mask) >= prefix survives.  An open column after the last pass keeps the first kk entries equal to prefix.
struct pprc_col { uint32_t prefix, mask; int32_t kk, done; };

// the entries of the lane's column over the rows [r0, r1), ascending: f(row, bits)
template <class F>
__device__ __forceinline__ void pprc_sweep(const uint32_t* __restrict__ Pc, int64_t B, int64_t r0, int64_t r1, F f) {
    int64_t r = r0;
    for (; r + GM_PPRC_UNROLL <= r1; r += GM_PPRC_UNROLL) {
        uint32_t b[GM_PPRC_UNROLL];
#pragma unroll
        for (int i = 0; i < GM_PPRC_UNROLL; ++i) b[i] = Pc[(r + i) * B];
#pragma unroll
        for (int i = 0; i < GM_PPRC_UNROLL; ++i) f(r + i, b[i]);
    }
    for (; r < r1; ++r) f(r, Pc[r * B]);
}

// the wave's place in a sweep launch of slabs x wgs workgroups: its column and its row range
struct pprc_place { int32_t c, range; int64_t r0, r1; };
__device__ __forceinline__ pprc_place pprc_place_of(int32_t wgs, int32_t rpw, int64_t N) {
    const int32_t slab = (int32_t)blockIdx.x / wgs, part = (int32_t)blockIdx.x - slab * wgs;
    pprc_place w;
    w.c = slab * GM_WAVE + ((int32_t)threadIdx.x & (GM_WAVE - 1));
    w.range = part * GM_PPRC_WAVES + ((int32_t)threadIdx.x >> 6);
    w.r0 = (int64_t)w.range * rpw;
    w.r0 = w.r0 < N ? w.r0 : N;
    w.r1 = w.r0 + rpw < N ? w.r0 + rpw : N;
    return w;
}

__global__ void __launch_bounds__(GM_CAND_THREADS) k_pprc_init(pprc_col* __restrict__ st, int32_t* __restrict__ cnt, int32_t B, int32_t k) {
    const int32_t c = (int32_t)(blockIdx.x * GM_CAND_THREADS + threadIdx.x);
    if (c >= B) return;
    st[c] = {0u, 0u, k, 0};
    cnt[c] = 0;
}

// a wave per column: +0.0f over the source's own entry and its neighbours' (src < 0: a column without a source, all zero already)
__global__ void __launch_bounds__(GM_CAND_THREADS) k_pprc_exclude(gm_nbr_graph G, const int32_t* __restrict__ src, int32_t B, float* __restrict__ P) {
    const int32_t c = (int32_t)(blockIdx.x * GM_CAND_WAVES + (threadIdx.x >> 6)), lane = (int32_t)threadIdx.x & (GM_WAVE - 1);
    if (c >= B) return;
    const int32_t a = src[c];
    if (a < 0 || a >= G.N) return;
    const int64_t a0 = G.ptr[a];
    const int32_t da = (int32_t)(G.ptr[a + 1] - a0);
    if (lane == 0) P[(int64_t)a * B + c] = 0.f;
    for (int32_t i = lane; i < da; i += GM_WAVE) P[(int64_t)G.idx[a0 + i] * B + c] = 0.f;
}

// one pass of the radix select: ghist[digit, c] += the open column's positive entries that carry the prefix, by their eight bits at `shift`
__global__ void __launch_bounds__(GM_PPRC_THREADS) k_pprc_hist(const uint32_t* __restrict__ P, int32_t B, int64_t N, int32_t wgs, int32_t rpw, int shift,
                                                               const pprc_col* __restrict__ st, int32_t* __restrict__ ghist) {
    __shared__ int32_t hist[GM_PPRC_BINS * GM_WAVE];                            // [bin][column of the slab]
    const pprc_place w = pprc_place_of(wgs, rpw, N);
    const pprc_col S = st[w.c];
    if (__all(S.done)) return;                                                  // (the same answer in every wave of the workgroup: they share the slab)
    const int tid = (int)threadIdx.x, lane = tid & (GM_WAVE - 1);
    for (int i = tid; i < GM_PPRC_BINS * GM_WAVE; i += GM_PPRC_THREADS) hist[i] = 0;
    __syncthreads();
    if (!S.done)
        pprc_sweep(P + w.c, B, w.r0, w.r1, [&](int64_t, uint32_t b) {
            if ((int32_t)b > 0 && (b & S.mask) == S.prefix) atomicAdd(&hist[(int)((b >> shift) & 255u) * GM_WAVE + lane], 1);
        });
    __syncthreads();
    const int32_t c0 = w.c - lane;
    for (int i = tid; i < GM_PPRC_BINS * GM_WAVE; i += GM_PPRC_THREADS) {
        const int32_t v = hist[i];
        if (v) atomicAdd(&ghist[(int64_t)(i >> 6) * B + c0 + (i & (GM_WAVE - 1))], v);
    }
}

// a workgroup per column: the digit that holds the kk-th largest of the counted entries; the column's bins are zero again behind it.  first: the pass
// over every positive entry -- their number is the total, and a set of at most k survives whole
__global__ void __launch_bounds__(GM_CAND_THREADS) k_pprc_pick(int32_t B, int shift, int first, int32_t k, pprc_col* __restrict__ st, int32_t* __restrict__ ghist,
                                                               int32_t* __restrict__ total) {
    __shared__ int part[GM_CAND_WAVES];
    const int tid = (int)threadIdx.x;
    const int32_t c = (int32_t)blockIdx.x;
    const pprc_col S = st[c];
    if (S.done) return;
    // thread t looks at digit 255 - t: the inclusive prefix counts the entries of this digit and above
    const int64_t at = (int64_t)(255 - tid) * B + c;
    const int h = ghist[at];
    ghist[at] = 0;
    int tot;
    const int inc = gm_cand_scan(h, part, &tot);                                // (its barriers stand between the loads of st[c] above and the store below)
    if (first) {
        if (tid == 0) total[c] = tot;
        if (tot <= k) {
            if (tid == 0) st[c] = {0u, 0u, 0, 1};
            return;
        }
    }
    if (inc - h < S.kk && S.kk <= inc) {                                        // exactly one thread
        const int32_t need = S.kk - (inc - h);
        st[c] = {S.prefix | ((uint32_t)(255 - tid) << shift), S.mask | (0xFFu << shift), need, need == h ? 1 : 0};      // the whole bin survives: done
    }
}

// ties[range, c] = the entries of the range equal to the threshold score of a column that is still open
__global__ void __launch_bounds__(GM_PPRC_THREADS) k_pprc_ties(const uint32_t* __restrict__ P, int32_t B, int64_t N, int32_t wgs, int32_t rpw, const pprc_col* __restrict__ st,
                                                               int32_t* __restrict__ ties) {
    const pprc_place w = pprc_place_of(wgs, rpw, N);
    const pprc_col S = st[w.c];
    if (S.done) return;
    int32_t n = 0;
    pprc_sweep(P + w.c, B, w.r0, w.r1, [&](int64_t, uint32_t b) { n += b == S.prefix ? 1 : 0; });
    ties[(int64_t)w.range * B + w.c] = n;
}

// a workgroup per open column: ties[., c] over the W ranges -> their exclusive prefix
__global__ void __launch_bounds__(GM_CAND_THREADS) k_pprc_tie_scan(int32_t B, int32_t W, const pprc_col* __restrict__ st, int32_t* __restrict__ ties) {
    __shared__ int part[GM_CAND_WAVES];
    const int tid = (int)threadIdx.x;
    const int32_t c = (int32_t)blockIdx.x;
    if (st[c].done) return;
    const int32_t per = (W + GM_CAND_THREADS - 1) / GM_CAND_THREADS;
    const int32_t lo = min(tid * per, W), hi = min(lo + per, W);
    int sum = 0;
    for (int32_t r = lo; r < hi; ++r) sum += ties[(int64_t)r * B + c];
    int tot;
    int run = gm_cand_scan(sum, part, &tot) - sum;
    for (int32_t r = lo; r < hi; ++r) {
        const int64_t at = (int64_t)r * B + c;
        const int32_t t = ties[at];
        ties[at] = run;
        run += t;
    }
}

// the survivors' keys -> surv[c, slot]: every entry above the threshold digits; AT them all of a closed column, of an open one the range's share of the
// first kk in row order
__global__ void __launch_bounds__(GM_PPRC_THREADS) k_pprc_collect(const uint32_t* __restrict__ P, int32_t B, int64_t N, int32_t wgs, int32_t rpw, const pprc_col* __restrict__ st,
                                                                  const int32_t* __restrict__ ties, int32_t* __restrict__ cnt, unsigned long long* __restrict__ surv) {
    const pprc_place w = pprc_place_of(wgs, rpw, N);
    const pprc_col S = st[w.c];
    int32_t left = 0;                                                           // open column: threshold entries this range may still keep
    if (!S.done) { left = S.kk - ties[(int64_t)w.range * B + w.c]; left = left > 0 ? left : 0; }
    unsigned long long* __restrict__ mine = surv + (int64_t)w.c * GM_CAND_MAX_K;
    pprc_sweep(P + w.c, B, w.r0, w.r1, [&](int64_t r, uint32_t b) {
        if ((int32_t)b <= 0) return;
        const uint32_t mb = b & S.mask;
        bool keep = mb > S.prefix;
        if (mb == S.prefix) {
            keep = S.done || left > 0;
            if (!S.done && left > 0) --left;
        }
        if (keep) {
            const int slot = atomicAdd(&cnt[w.c], 1);
            if (slot < GM_CAND_MAX_K) mine[slot] = gm_cand_key(b, (int32_t)r);
        }
    });
}

// block i: output row row[i] from the column col[i] - c0 of the round (col < 0: a source outside the graph -- total 0, all padding)
__global__ void __launch_bounds__(GM_CAND_THREADS) k_pprc_out(const int32_t* __restrict__ row, const int32_t* __restrict__ col, int64_t c0, int32_t k, const int32_t* __restrict__ cnt,
                                                              const int32_t* __restrict__ total, const unsigned long long* __restrict__ surv, int32_t* __restrict__ out_nodes,
                                                              float* __restrict__ out_scores, int32_t* __restrict__ out_total) {
    __shared__ unsigned long long sk[GM_CAND_MAX_K];
    const int tid = (int)threadIdx.x;
    const int64_t r = row[blockIdx.x];
    const int64_t c = col[blockIdx.x] < 0 ? -1 : (int64_t)col[blockIdx.x] - c0;
    const int n = c < 0 ? 0 : min(cnt[c], GM_CAND_MAX_K);                       // = min(k, total)
    for (int i = tid; i < n; i += GM_CAND_THREADS) sk[i] = surv[c * GM_CAND_MAX_K + i];
    __syncthreads();
    gm_cand_sort_write(sk, n, k, r * (int64_t)k, out_nodes, out_scores);
    if (tid == 0) out_total[r] = c < 0 ? 0 : total[c];
}

int gm_pprc_prepare(gm_pprc* w, gm_scratch& sc, int32_t Bmax, int32_t k, hipStream_t st) {
    w->k = k; w->st = st; w->wgs_max = 2 * gm_num_cus();
    if (!Bmax) return GM_OK;
    pprc_col* cols = nullptr;
    GM_TRY(sc.take(&cols, (size_t)Bmax));
    w->cols = cols;
    GM_TRY(sc.take(&w->hist, (size_t)GM_PPRC_BINS * (size_t)Bmax));
    GM_TRY(sc.take(&w->cnt, (size_t)Bmax));
    GM_TRY(sc.take(&w->total, (size_t)Bmax));
    GM_TRY(sc.take(&w->ties, (size_t)(w->wgs_max + Bmax / GM_WAVE) * GM_PPRC_WAVES * GM_WAVE));      // ranges x columns of any round: (wgs_max / slabs + 1) x 8 ranges x 64 slabs columns
    GM_TRY(sc.take(&w->surv, (size_t)Bmax * GM_CAND_MAX_K));
    GM_HIP(hipMemsetAsync(w->hist, 0, (size_t)GM_PPRC_BINS * (size_t)Bmax * sizeof(int32_t), st));      // every pick leaves its bins zero behind it
    return GM_OK;
}

int gm_pprc_round(const gm_pprc& w, const gm_nbr_graph& G, float* P, int32_t Br, const int32_t* d_src, const int32_t* d_row, const int32_t* d_col, int64_t c0, int64_t rows,
                  int32_t* d_out_nodes, float* d_out_scores, int32_t* d_out_total, gm_phase_timer* tm) {
    hipStream_t st = w.st;
    pprc_col* cols = (pprc_col*)w.cols;
    if (tm) { GM_HIP(hipStreamSynchronize(st)); tm->lap("walk"); }
    if (Br) {
        const int32_t slabs = Br / GM_WAVE;
        // the sweeps' grid: about two workgroups per CU over all slabs, a range never below GM_PPRC_MIN_ROWS rows
        const int64_t by_rows = (G.N + (int64_t)GM_PPRC_MIN_ROWS * GM_PPRC_WAVES - 1) / ((int64_t)GM_PPRC_MIN_ROWS * GM_PPRC_WAVES);
        const int32_t wgs = (int32_t)std::max<int64_t>(1, std::min<int64_t>((w.wgs_max + slabs - 1) / slabs, by_rows));
        const int32_t W = wgs * GM_PPRC_WAVES;
        const int32_t rpw = (int32_t)((G.N + W - 1) / W);
        const dim3 sweep((unsigned)(slabs * wgs)), sweep_block(GM_PPRC_THREADS), per_col((unsigned)Br), block(GM_CAND_THREADS);
        const uint32_t* Pb = (const uint32_t*)P;
        hipLaunchKernelGGL(k_pprc_init, dim3((unsigned)((Br + GM_CAND_THREADS - 1) / GM_CAND_THREADS)), block, 0, st, cols, w.cnt, Br, w.k);
        hipLaunchKernelGGL(k_pprc_exclude, dim3((unsigned)((Br + GM_CAND_WAVES - 1) / GM_CAND_WAVES)), block, 0, st, G, d_src, Br, P);
        GM_HIP(hipGetLastError());
        if (tm) { GM_HIP(hipStreamSynchronize(st)); tm->lap("exclusion"); }
        for (int shift = 24; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(k_pprc_hist, sweep, sweep_block, 0, st, Pb, Br, G.N, wgs, rpw, shift, (const pprc_col*)cols, w.hist);
            hipLaunchKernelGGL(k_pprc_pick, per_col, block, 0, st, Br, shift, shift == 24 ? 1 : 0, w.k, cols, w.hist, w.total);
        }
        hipLaunchKernelGGL(k_pprc_ties, sweep, sweep_block, 0, st, Pb, Br, G.N, wgs, rpw, (const pprc_col*)cols, w.ties);
        hipLaunchKernelGGL(k_pprc_tie_scan, per_col, block, 0, st, Br, W, (const pprc_col*)cols, w.ties);
        hipLaunchKernelGGL(k_pprc_collect, sweep, sweep_block, 0, st, Pb, Br, G.N, wgs, rpw, (const pprc_col*)cols, (const int32_t*)w.ties, w.cnt, w.surv);
        GM_HIP(hipGetLastError());
    }
    if (rows) {
        hipLaunchKernelGGL(k_pprc_out, dim3((unsigned)rows), dim3(GM_CAND_THREADS), 0, st, d_row, d_col, c0, w.k, (const int32_t*)w.cnt, (const int32_t*)w.total,
                           (const unsigned long long*)w.surv, d_out_nodes, d_out_scores, d_out_total);
        GM_HIP(hipGetLastError());
    }
    if (tm) { GM_HIP(hipStreamSynchronize(st)); tm->lap("select"); }
    return GM_OK;
}
