// Candidate partners for link prediction (gm_store_pair_candidates): per source node the non-adjacent nodes that share a neighbour with it, ranked by
// one of the pair scores, the best k returned.  The DEFINITION -- candidate set, score, ranking key, padding -- is in include/gmeta_hip.h;
// tests/candidate_ref.py restates it with Python sets and the GPU tests compare nodes, score bits and totals for equality.  This file is how it is computed:
//   enumerate   k_cand_walk: one workgroup per source a, a membership bitmap over the graph's N nodes in LDS (up to GM_CAND_LDS_WORDS words = 32 KiB, N <= 262,144:
//               four resident workgroups per CU at the bound, seven at the 21 KiB of the arxiv shape) or, above that, in a per-workgroup slab of HBM that
//               a fixed grid of workgroups strides the sources with (agent-scope atomics, as extract.hip's k_nodes does for large parents).  The workgroup
//               walks Gamma(a) and, for every z in it, Gamma(z) in the neighbour index, setting bits: rows are latency chains, so a group of 8 lanes takes
//               one z (32 rows in flight per workgroup) and a row above GM_CAND_LONG entries goes to a whole wave.  Then the bits of Gamma(a) and of a are
//               cleared, every thread counts a contiguous run of words, and a block scan turns the counts into positions.  The walk runs twice: a COUNT pass
//               over all sources writes |C(a)| (d_out_total; the host reads it and cuts the rounds by exact sizes), a FILL pass per round writes the
//               (a, w) pairs, w ascending, at the source's offset.  Both leave the bitmap zero behind them.
//   score       the existing k_pair_scores<LPP> on the round's pairs, through gm_pair_scores_launch (pair_scores.hip): the same instructions on the same
//               pairs as gm_store_pair_scores, so the bits are its bits.
//   select      k_cand_select: one workgroup per source over its segment.  The 64-bit key (score bits << 32 | 0xFFFFFFFF - w) is formed on the fly from the
//               pair and score tables; keys are unique.  A segment longer than k gets a radix select of the k-th largest key, eight bits a pass from the
//               top (a 256-bin LDS histogram of integer counts; it stops as soon as the chosen bin is wanted whole), then the survivors (at most 1,024) are
//               sorted in LDS by a bitonic network and written with the padding.  Which slot a survivor lands in before the sort depends on arrival; the
//               sorted order of unique keys does not.  The key, the workgroup scan and the sort with the padding are in gm_internal.h (gm_cand_*): the
//               PageRank candidates (pagerank_candidates.hip) rank with the same code.
// Everything runs on the caller's stream; scratch comes from the stream-ordered pool and goes back to it on that stream.  No float arithmetic at all here,
// no scratch memory in the kernels, integer atomics only where the result cannot depend on their order (bit sets, histogram counts).
#include "gm_nbr.h"
#include "gm_devutil.h"      // wld / wst: the bitmap words in LDS (G = false) or in the workgroup's slab of HBM (G = true, agent-scope atomics: L1 is not coherent with the atomics that set the bits)

#define GM_CAND_GROUP 8                   // lanes per neighbour row of the walk
#define GM_CAND_LONG 128                  // rows above this many entries are walked by a whole wave
#define GM_CAND_LDS_WORDS 8192            // bitmap words in LDS at most: 32 KiB, N <= 262,144
#define GM_CAND_COLS 5
#define GM_CAND_ROUND_DEFAULT (1 << 22)   // pairs per round: 28 bytes of scratch each (the pair and its five scores)

// the graph's view and the length of a membership bitmap over its nodes
struct cand_graph {
    gm_nbr_graph g;
    int32_t words;               // ceil(N / 32); the host has checked N <= INT32_MAX
};

template <bool G> __device__ __forceinline__ void cw_sync() {
    if (G) __threadfence();
    __syncthreads();
}

// FILL = false: total[r] = |C(nodes[r])|.  FILL = true: pairs[2 (off[r] + j)] = (nodes[r], j-th candidate, ascending).  The bitmap is zero on entry
// (LDS: cleared here; slab: by the host, once) and zero again behind every source.
template <bool G, bool FILL>
__global__ void __launch_bounds__(GM_CAND_THREADS)
k_cand_walk(cand_graph Gr, const int32_t* __restrict__ nodes, int32_t m, uint32_t* slab, const int32_t* __restrict__ off, int32_t* __restrict__ total, int32_t* __restrict__ pairs) {
    extern __shared__ uint32_t lds_bm[];
    __shared__ int part[GM_CAND_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & (GM_WAVE - 1), wave = tid / GM_WAVE;
    const int grp = tid / GM_CAND_GROUP, gl = tid & (GM_CAND_GROUP - 1);
    const gm_nbr_graph& Nb = Gr.g;
    const int32_t N = (int32_t)Nb.N;
    const int words = Gr.words;
    uint32_t* bm = G ? slab + (int64_t)blockIdx.x * words : lds_bm;
    if (!G) {
        for (int w = tid; w < words; w += GM_CAND_THREADS) bm[w] = 0u;
        __syncthreads();
    }
    const int wpt = (words + GM_CAND_THREADS - 1) / GM_CAND_THREADS;             // every thread owns a contiguous run of words: ascending ids from one scan
    const int w0 = min(tid * wpt, words), w1 = min(w0 + wpt, words);
    for (int32_t r = (int32_t)blockIdx.x; r < m; r += (int32_t)gridDim.x) {
        const int32_t a = nodes[r];
        if (a < 0 || a >= N) {                                                  // a source outside the graph: C is empty (uniform over the workgroup)
            if (!FILL && tid == 0) total[r] = 0;
            continue;
        }
        const int64_t a0 = Nb.ptr[a];
        const int32_t da = (int32_t)(Nb.ptr[a + 1] - a0);
        const int32_t* __restrict__ row = Nb.idx + a0;
        // short rows: one per group of eight lanes
        for (int32_t i = grp; i < da; i += GM_CAND_THREADS / GM_CAND_GROUP) {
            const int32_t z = row[i];
            const int64_t z0 = Nb.ptr[z];
            const int32_t dz = (int32_t)(Nb.ptr[z + 1] - z0);
            if (dz > GM_CAND_LONG) continue;
            for (int32_t j = gl; j < dz; j += GM_CAND_GROUP) { const int32_t w = Nb.idx[z0 + j]; atomicOr(&bm[w >> 5], 1u << (w & 31)); }
        }
        // long rows: the waves take them in turn, 64 lanes a row
        int seen = 0;
        for (int32_t base = 0; base < da; base += GM_WAVE) {
            const int32_t i = base + lane;
            int64_t z0 = 0; int32_t dz = 0;
            if (i < da) { const int32_t z = row[i]; z0 = Nb.ptr[z]; dz = (int32_t)(Nb.ptr[z + 1] - z0); }
            unsigned long long ml = __ballot(dz > GM_CAND_LONG);
            while (ml) {
                const int b = __ffsll((long long)ml) - 1;
                ml &= ml - 1ull;
                if ((seen++ & (GM_CAND_WAVES - 1)) != wave) continue;
                const int64_t s0 = __shfl(z0, b, GM_WAVE);
                const int32_t ds = __shfl(dz, b, GM_WAVE);
                for (int32_t j = lane; j < ds; j += GM_WAVE) { const int32_t w = Nb.idx[s0 + j]; atomicOr(&bm[w >> 5], 1u << (w & 31)); }
            }
        }
        cw_sync<G>();
        // C(a) holds neither a neighbour of a nor a itself
        for (int32_t i = tid; i < da; i += GM_CAND_THREADS) { const int32_t z = row[i]; atomicAnd(&bm[z >> 5], ~(1u << (z & 31))); }
        if (tid == 0) atomicAnd(&bm[a >> 5], ~(1u << (a & 31)));
        cw_sync<G>();
        int c = 0;
        for (int w = w0; w < w1; ++w) c += __popc(wld<G>(&bm[w]));
        int tot;
        const int inc = gm_cand_scan(c, part, &tot);
        if (!FILL) {
            if (tid == 0) total[r] = tot;
            for (int w = w0; w < w1; ++w) wst<G>(&bm[w], 0u);
        } else {
            int64_t pos = (int64_t)off[r] + (inc - c);
            for (int w = w0; w < w1; ++w) {
                uint32_t bits = wld<G>(&bm[w]);
                while (bits) {
                    const int b = __ffs((int)bits) - 1;
                    bits &= bits - 1u;
                    pairs[2 * pos] = a; pairs[2 * pos + 1] = w * 32 + b;
                    ++pos;
                }
                wst<G>(&bm[w], 0u);
            }
        }
        cw_sync<G>();                                                           // the bitmap is zero before the next source sets a bit
    }
}

__device__ __forceinline__ unsigned long long cand_key(const int32_t* __restrict__ pairs, const float* __restrict__ scores, int col, int64_t i) {
    return gm_cand_key(__float_as_uint(scores[GM_CAND_COLS * i + col]), pairs[2 * i + 1]);
}

// block r: the segment [off[r], off[r + 1]) of the round's pairs -> row r0 + r of the result
__global__ void __launch_bounds__(GM_CAND_THREADS)
k_cand_select(const int32_t* __restrict__ pairs, const float* __restrict__ scores, int col, const int32_t* __restrict__ off, int64_t r0, int k,
              int32_t* __restrict__ out_nodes, float* __restrict__ out_scores) {
    __shared__ unsigned long long sk[GM_CAND_MAX_K];
    __shared__ int hist[256];
    __shared__ int part[GM_CAND_WAVES];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_k, s_done, s_cnt;
    const int tid = (int)threadIdx.x;
    const int64_t b = off[blockIdx.x], e = off[blockIdx.x + 1];
    unsigned long long T = 0ull;                                                // survivors: key >= T
    if (e - b > k) {
        unsigned long long prefix = 0ull, mask = 0ull;
        int kk = k;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;                                                      // (256 threads, 256 bins)
            __syncthreads();
            for (int64_t i = b + tid; i < e; i += GM_CAND_THREADS) {
                const unsigned long long key = cand_key(pairs, scores, col, i);
                if ((key & mask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
            }
            __syncthreads();
            // thread t looks at digit 255 - t: the inclusive prefix counts the keys of this digit and above
            const int h = hist[255 - tid];
            int tot;
            const int inc = gm_cand_scan(h, part, &tot);
            if (inc - h < kk && kk <= inc) {                                    // exactly one thread: the digit that holds the kk-th largest
                s_prefix = prefix | ((unsigned long long)(255 - tid) << shift);
                s_k = kk - (inc - h);
                s_done = (kk - (inc - h)) == h;                                 // the whole bin survives: nothing below this digit decides anything
            }
            __syncthreads();
            prefix = s_prefix; kk = s_k; mask |= 0xFFull << shift;
            const int done = s_done;
            __syncthreads();
            if (done) break;
        }
        T = prefix;
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int64_t i = b + tid; i < e; i += GM_CAND_THREADS) {
        const unsigned long long key = cand_key(pairs, scores, col, i);
        if (key >= T) { const int slot = atomicAdd(&s_cnt, 1); if (slot < GM_CAND_MAX_K) sk[slot] = key; }
    }
    __syncthreads();
    const int cnt = min(s_cnt, GM_CAND_MAX_K);                                  // = min(k, e - b)
    gm_cand_sort_write(sk, cnt, k, (r0 + blockIdx.x) * (int64_t)k, out_nodes, out_scores);
}

template <bool FILL>
static void cand_launch_walk(bool hbm, unsigned grid, size_t lds, hipStream_t st, const cand_graph& G, const int32_t* nodes, int32_t m, uint32_t* slab, const int32_t* off,
                             int32_t* total, int32_t* pairs) {
    if (hbm) hipLaunchKernelGGL((k_cand_walk<true, FILL>), dim3(grid), dim3(GM_CAND_THREADS), 0, st, G, nodes, m, slab, off, total, pairs);
    else hipLaunchKernelGGL((k_cand_walk<false, FILL>), dim3(grid), dim3(GM_CAND_THREADS), lds, st, G, nodes, m, slab, off, total, pairs);
}

extern "C" int32_t gm_store_pair_candidates(const gm_store_t* s, int32_t g, const int32_t* d_nodes, int64_t m, int32_t k, int32_t col, int32_t* d_out_nodes,
                                            float* d_out_scores, int32_t* d_out_total, void* stream) {
    const char* what = "gm_store_pair_candidates";
    GM_TRY(gm_store_call_check(what, s, g, "m", m));
    GM_REQUIRE(k >= 1 && k <= GM_CAND_MAX_K, GM_EINVAL, "%s: k = %d; 1 .. %d", what, k, GM_CAND_MAX_K);
    GM_REQUIRE(col >= 0 && col < GM_CAND_COLS, GM_EINVAL, "%s: col = %d; 0 .. 4 (cn, jaccard, adamic_adar, resource_allocation, pref_attachment)", what, col);
    GM_TRY(gm_pair_lanes(s, g, what, nullptr));
    const int home = gm_knob().cand_bitmap, budget_knob = gm_knob().cand_round;
    GM_REQUIRE(home >= 0 && home <= 2, GM_EINVAL, "%s: cand_bitmap = %d; 0 (the library's choice), 1 (LDS) or 2 (HBM slab)", what, home);
    GM_REQUIRE(budget_knob >= 0, GM_EINVAL, "%s: cand_round = %d", what, budget_knob);
    const int64_t N = s->node_off[g + 1] - s->node_off[g];
    GM_REQUIRE(N <= (int64_t)INT32_MAX, GM_ERANGE, "%s: graph %d has %lld nodes", what, g, (long long)N);
    const int32_t words = (int32_t)((N + 31) / 32);
    GM_REQUIRE(!(home == 1 && words > GM_CAND_LDS_WORDS), GM_EINVAL, "%s: cand_bitmap = 1 (LDS) but graph %d has %lld nodes; the LDS bitmap holds %d at most", what, g,
               (long long)N, GM_CAND_LDS_WORDS * 32);
    if (m == 0) return GM_OK;
    GM_REQUIRE(d_nodes && d_out_nodes && d_out_scores && d_out_total, GM_EINVAL, "%s: NULL argument", what);
    GM_TRY(gm_nbr_index(s));
    int lpp = 0;
    GM_TRY(gm_pair_lanes(s, g, what, &lpp));
    hipStream_t st = (hipStream_t)stream;
    gm_phase_timer tm("pair candidates");
    const bool timed = gm_knob().timing != 0;
    const bool hbm = home == 2 || words > GM_CAND_LDS_WORDS;
    const cand_graph G = {gm_nbr_graph_of(s, g), words};
    const size_t lds = hbm ? 0 : (size_t)(words ? words : 1) * sizeof(uint32_t);
    const int64_t slabs = std::min<int64_t>(m, 2 * (int64_t)gm_num_cus());     // HBM home: a fixed grid strides the sources, one slab a workgroup
    const unsigned walk_grid = (unsigned)(hbm ? slabs : m);

    gm_scratch sc(st);
    uint32_t* slab = nullptr;
    if (hbm) {
        GM_TRY(sc.take(&slab, (size_t)slabs * (size_t)words));
        GM_HIP(hipMemsetAsync(slab, 0, (size_t)slabs * (size_t)words * sizeof(uint32_t), st));
    }
    // the count pass over every source; the host cuts the rounds by the exact set sizes
    cand_launch_walk<false>(hbm, walk_grid, lds, st, G, d_nodes, (int32_t)m, slab, nullptr, d_out_total, nullptr);
    GM_HIP(hipGetLastError());
    gm_stager sg(st);
    const int32_t* h_total = sg.download(d_out_total, (size_t)m);
    GM_REQUIRE(h_total, GM_ENOMEM, "%s: pinned staging allocation failed", what);
    GM_HIP(hipStreamSynchronize(st));
    tm.lap("enumerate");

    const int64_t budget = budget_knob > 0 ? budget_knob : GM_CAND_ROUND_DEFAULT;
    struct round { int64_t r0, r1, pairs; };
    std::vector<round> rounds;
    int64_t max_pairs = 0, max_src = 0;
    for (int64_t r0 = 0; r0 < m;) {
        int64_t r1 = r0, sum = 0;
        while (r1 < m && !(r1 > r0 && sum + h_total[r1] > budget)) sum += h_total[r1++];     // a source above the budget: a round of its own
        GM_REQUIRE(sum <= (int64_t)INT32_MAX, GM_ERANGE, "%s: a round of %lld pairs; the kernels count in int32", what, (long long)sum);
        rounds.push_back({r0, r1, sum});
        max_pairs = std::max(max_pairs, sum); max_src = std::max(max_src, r1 - r0);
        r0 = r1;
    }
    int32_t* pairs = nullptr; float* scores = nullptr; int32_t* off = nullptr;
    GM_TRY(sc.take(&pairs, (size_t)max_pairs * 2));
    GM_TRY(sc.take(&scores, (size_t)max_pairs * GM_CAND_COLS));
    GM_TRY(sc.take(&off, (size_t)(max_src + 1)));

    std::vector<int32_t> h_off;
    for (const round& R : rounds) {
        const int64_t ms = R.r1 - R.r0;
        h_off.assign((size_t)ms + 1, 0);
        for (int64_t r = 0; r < ms; ++r) h_off[r + 1] = h_off[r] + h_total[R.r0 + r];
        GM_TRY(sg.upload(off, h_off));
        if (R.pairs > 0) {
            cand_launch_walk<true>(hbm, (unsigned)std::min<int64_t>(walk_grid, ms), lds, st, G, d_nodes + R.r0, (int32_t)ms, slab, off, nullptr, pairs);
            GM_HIP(hipGetLastError());
            if (timed) { GM_HIP(hipStreamSynchronize(st)); tm.lap("enumerate"); }
            GM_TRY(gm_pair_scores_launch(s, g, lpp, pairs, R.pairs, 0, scores, st));
            if (timed) { GM_HIP(hipStreamSynchronize(st)); tm.lap("score"); }
        }
        hipLaunchKernelGGL(k_cand_select, dim3((unsigned)ms), dim3(GM_CAND_THREADS), 0, st, (const int32_t*)pairs, (const float*)scores, (int)col, (const int32_t*)off, R.r0, (int)k,
                           d_out_nodes, d_out_scores);
        GM_HIP(hipGetLastError());
        if (timed) { GM_HIP(hipStreamSynchronize(st)); tm.lap("select"); }
    }
    GM_HIP(hipStreamSynchronize(st));
    return GM_OK;
}
