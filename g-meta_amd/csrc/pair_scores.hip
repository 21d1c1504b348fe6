// Neighbourhood heuristic scores of node pairs (gm_store_pair_scores: common neighbours, Jaccard, Adamic-Adar, resource allocation, preferential
// attachment) over the neighbour index (nbr_index.hip; gm_nbr.h).  The DEFINITION is in include/gmeta_hip.h; tests/pair_score_ref.py restates it with
// Python sets and fp64 sums.  This file is how it is computed:
//   the scores  k_pair_scores<LPP>: LPP lanes per pair, 64 / LPP pairs per wave.  The group strides over the SHORTER of the two rows and each lane
//               binary-searches its id in the longer one (gm_nbr_common) and gathers the two node terms on a hit.  Lane partials meet in a butterfly over the
//               group: a fixed order, every lane ends with the same bits, no atomics.  The mask test is one more search (gm_nbr_adjacent).
//               Integer and latency work, as the negative sampler is: the host picks LPP per launch from the graph's mean distinct degree
//               (gm_set_tuning("pair_lanes") forces one).
#include "gm_nbr.h"

#define GM_PAIR_THREADS 256
#define GM_PAIR_COLS 5

// the graph's view and its two per-node term tables
struct pair_graph {
    gm_nbr_graph g;
    const float* aa;             // gm_store::d_nbr_aa + node_off[g]    [N]
    const float* ra;             // gm_store::d_nbr_ra + node_off[g]    [N]
};

struct pair_sums { int32_t cn; float aa, ra; };      // a lane's share of the common neighbours: their number and the sums of their two terms

template <int LPP>
__global__ void __launch_bounds__(GM_PAIR_THREADS) k_pair_scores(pair_graph G, const int32_t* __restrict__ pairs, int64_t n, int mask, float* __restrict__ out) {
    const int64_t p = ((int64_t)blockIdx.x * GM_PAIR_THREADS + threadIdx.x) / LPP;      // the group's pair: a group is live or idle as a whole
    const int lane = (int)threadIdx.x & (LPP - 1);
    const bool live = p < n;
    int32_t cn = 0, da = 0, db = 0;
    float aa = 0.f, ra = 0.f;
    bool self = false;
    if (live) {
        const gm_nbr_pair w = gm_nbr_pair_of(G.g, pairs, p);
        if (w.in) {                                                                      // a node outside the graph: five zeros
            self = w.u == w.v; da = w.du; db = w.dv;
            const pair_sums t = gm_nbr_common<LPP>(w.X, w.dx, w.T, w.dt, lane, pair_sums{0, 0.f, 0.f}, [&](pair_sums t, int32_t z) {
                ++t.cn; t.aa += G.aa[z]; t.ra += G.ra[z];
                return t;
            });
            cn = t.cn; aa = t.aa; ra = t.ra;
            if (mask && gm_nbr_adjacent(w)) { --da; --db; }
        }
    }
#pragma unroll
    for (int m = LPP / 2; m >= 1; m >>= 1) {
        cn += __shfl_xor(cn, m, LPP); aa += __shfl_xor(aa, m, LPP); ra += __shfl_xor(ra, m, LPP);
    }
    if (!live || lane >= GM_PAIR_COLS) return;
    const int64_t U = self ? (int64_t)da : (int64_t)da + db - cn;
    const float val = lane == 0 ? (float)cn : lane == 1 ? (U > 0 ? __fdiv_rn((float)cn, (float)U) : 0.f) : lane == 2 ? aa : lane == 3 ? ra : (float)((int64_t)da * (int64_t)db);
    out[GM_PAIR_COLS * p + lane] = val;
}

// Lanes per pair: the group strides the shorter row, so a wide group idles on a sparse graph and a narrow one walks a dense row in many steps.  Measured on
// preferential-attachment graphs, |E| / 2 edges + as many negatives (profiles/pair_scores.txt): 16 lanes are fastest from a mean distinct degree of 2 up to 80
// (an 8-lane group never won: eight diverging searches per wave cost more than the idle lanes of four), 16 and 32 level at 146, 32 and 64 level at 287, 64 ahead at 554
static int pair_lanes_for(const gm_store* s, int32_t g) {
    const int64_t N = s->node_off[g + 1] - s->node_off[g], nnz = s->nbr_off[g + 1] - s->nbr_off[g];
    return nnz <= 192 * N ? 16 : nnz <= 384 * N ? 32 : 64;
}

int gm_pair_lanes(const gm_store* s, int32_t g, const char* what, int* lpp) {
    const int forced = gm_knob().pair_lanes;
    GM_REQUIRE(forced == 0 || forced == 16 || forced == 32 || forced == 64, GM_EINVAL,
               "%s: pair_lanes = %d; the kernel is built for 16, 32 and 64 lanes per pair (0: the library's choice)", what, forced);
    if (lpp) *lpp = forced ? forced : pair_lanes_for(s, g);
    return GM_OK;
}

int gm_pair_scores_launch(const gm_store* s, int32_t g, int lpp, const int32_t* d_pairs, int64_t n, int mask, float* d_out, hipStream_t st) {
    const pair_graph G = {gm_nbr_graph_of(s, g), s->d_nbr_aa + s->node_off[g], s->d_nbr_ra + s->node_off[g]};
    const dim3 grid((unsigned)((n * lpp + GM_PAIR_THREADS - 1) / GM_PAIR_THREADS)), block(GM_PAIR_THREADS);      // n <= 2^31 - 1 pairs of at most 64 lanes: below 2^29 blocks
    if (lpp == 16) hipLaunchKernelGGL(k_pair_scores<16>, grid, block, 0, st, G, d_pairs, n, mask, d_out);
    else if (lpp == 32) hipLaunchKernelGGL(k_pair_scores<32>, grid, block, 0, st, G, d_pairs, n, mask, d_out);
    else hipLaunchKernelGGL(k_pair_scores<64>, grid, block, 0, st, G, d_pairs, n, mask, d_out);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

extern "C" int32_t gm_store_pair_scores(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, float* d_out, void* stream) {
    const char* what = "gm_store_pair_scores";
    GM_TRY(gm_store_call_check(what, s, g, "n", n, flags));
    GM_TRY(gm_pair_lanes(s, g, what, nullptr));
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out, GM_EINVAL, "%s: NULL argument", what);
    GM_TRY(gm_nbr_index(s));
    int lpp = 0;
    GM_TRY(gm_pair_lanes(s, g, what, &lpp));                                             // (the library's choice reads the index's row lengths)
    return gm_pair_scores_launch(s, g, lpp, d_pairs, n, flags & GM_PAIR_MASK_TARGET, d_out, (hipStream_t)stream);
}
