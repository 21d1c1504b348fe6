// Neighbourhood heuristic scores of node pairs (gm_store_pair_scores: common neighbours, Jaccard, Adamic-Adar, resource allocation, preferential
// attachment) and the neighbour index they read (gm_store_neighbour_degrees shows its degrees).  The DEFINITION is in include/gmeta_hip.h;
// tests/pair_score_ref.py restates it with Python sets and fp64 sums.  This file is how it is computed:
//   the index   per node the ascending DISTINCT row of its in- and out-neighbours without itself (int64 row pointers over all graphs, int32 graph-local
//               ids) and deg, 1 / ln(deg), 1 / deg.  Built on the host at the first call that needs it: the in-rows of the store keep the caller's edge
//               order, so a merge needs a sort per row, and the build happens once per store.  It runs under gm_store::nbr_mu and the upload is complete on
//               the device before the lock is released, so every later call reads the index from whichever stream it runs on, with no event.
//   the scores  k_pair_scores<LPP>: LPP lanes per pair, 64 / LPP pairs per wave.  The group strides over the SHORTER of the two rows (consecutive lanes read
//               consecutive ids: one coalesced load per step), each lane binary-searches its id in the longer row -- log2(length) dependent loads, the
//               upper levels shared by the whole group in L1 / L2 -- and gathers the two node terms on a hit.  Lane partials meet in a butterfly over the
//               group: a fixed order, every lane ends with the same bits, no atomics.  The mask test is one more search, of b in a's row.
//               Integer and latency work, as the negative sampler is: the host picks LPP per launch from the graph's mean distinct degree
//               (gm_set_tuning("pair_lanes") forces one).
#include <math.h>
#include "gm_internal.h"

#define GM_PAIR_THREADS 256
#define GM_PAIR_COLS 5

// one parent graph of a store inside the neighbour index: rows by LOCAL node id, offsets global (into idx), neighbours local
struct pair_graph {
    const int64_t* ptr;          // gm_store::d_nbr_ptr + node_off[g]   [N + 1]
    const int32_t* idx;          // gm_store::d_nbr_idx
    const float* aa;             // gm_store::d_nbr_aa + node_off[g]    [N]
    const float* ra;             // gm_store::d_nbr_ra + node_off[g]    [N]
    int64_t N;
};

// v in the ascending row[0 .. len)
__device__ __forceinline__ bool nbr_has(const int32_t* __restrict__ row, int32_t len, int32_t v) {
    int32_t lo = 0, hi = len;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t x = row[mid];
        if (x == v) return true;
        if (x < v) lo = mid + 1; else hi = mid;
    }
    return false;
}

template <int LPP>
__global__ void __launch_bounds__(GM_PAIR_THREADS) k_pair_scores(pair_graph G, const int32_t* __restrict__ pairs, int64_t n, int mask, float* __restrict__ out) {
    const int64_t p = ((int64_t)blockIdx.x * GM_PAIR_THREADS + threadIdx.x) / LPP;      // the group's pair: a group is live or idle as a whole
    const int lane = (int)threadIdx.x & (LPP - 1);
    const bool live = p < n;
    int32_t a = -1, b = -1;
    if (live) { a = pairs[2 * p]; b = pairs[2 * p + 1]; }
    const bool in = a >= 0 && a < G.N && b >= 0 && b < G.N;                              // a node outside the graph: five zeros
    int32_t cn = 0, da = 0, db = 0;
    float aa = 0.f, ra = 0.f;
    bool self = false;
    if (in) {
        const int32_t u = a < b ? a : b, v = a < b ? b : a;                              // canonical: (a, b) and (b, a) run the same instructions on the same data
        self = u == v;
        const int64_t u0 = G.ptr[u], v0 = G.ptr[v];
        da = (int32_t)(G.ptr[u + 1] - u0); db = (int32_t)(G.ptr[v + 1] - v0);
        const bool u_short = da <= db;                                                   // a tie takes the smaller id's row
        const int32_t* __restrict__ S = G.idx + (u_short ? u0 : v0);
        const int32_t* __restrict__ L = G.idx + (u_short ? v0 : u0);
        const int32_t ns = u_short ? da : db, nl = u_short ? db : da;
        for (int32_t i = lane; i < ns; i += LPP) {
            const int32_t z = S[i];
            if (nbr_has(L, nl, z)) { ++cn; aa += G.aa[z]; ra += G.ra[z]; }
        }
        if (mask && !self && nbr_has(G.idx + u0, da, v)) { --da; --db; }                  // (v in u's row <=> u in v's row: the rows are symmetric)
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

// ---------------------------------------------------------------------------------------------------- the neighbour index
static void nbr_release(const gm_store* s) {
    gm_dev_free(s->d_nbr_ptr, nullptr); gm_dev_free(s->d_nbr_idx, nullptr); gm_dev_free(s->d_nbr_deg, nullptr); gm_dev_free(s->d_nbr_aa, nullptr); gm_dev_free(s->d_nbr_ra, nullptr);
    s->d_nbr_ptr = nullptr; s->d_nbr_idx = nullptr; s->d_nbr_deg = nullptr; s->d_nbr_aa = nullptr; s->d_nbr_ra = nullptr;
}

template <class T> static int nbr_upload(T** d, const std::vector<T>& v) {
    GM_TRY(gm_dev_alloc((void**)d, (v.empty() ? 1 : v.size()) * sizeof(T), nullptr));
    if (!v.empty()) GM_HIP(hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return GM_OK;
}

static int nbr_build(const gm_store* s) {
    gm_phase_timer tm("neighbour index");
    const int64_t T = s->total_nodes, E = s->total_edges;
    std::vector<int64_t> in_ptr(T + 1), out_ptr(T + 1);
    std::vector<int32_t> in_idx(E ? E : 1), out_idx(E ? E : 1);
    GM_HIP(hipMemcpy(in_ptr.data(), s->d_in_ptr, (T + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    GM_HIP(hipMemcpy(out_ptr.data(), s->d_out_ptr, (T + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (E) {
        GM_HIP(hipMemcpy(in_idx.data(), s->d_in_idx, E * sizeof(int32_t), hipMemcpyDeviceToHost));
        GM_HIP(hipMemcpy(out_idx.data(), s->d_out_idx, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    tm.lap("download");
    std::vector<int64_t> ptr(T + 1, 0), off(s->n_graphs + 1, 0);
    std::vector<int32_t> idx, deg(T), row;
    std::vector<float> aa(T), ra(T);
    idx.reserve((size_t)(2 * E));
    for (int g = 0; g < s->n_graphs; ++g) {
        for (int64_t x = s->node_off[g]; x < s->node_off[g + 1]; ++x) {
            const int32_t self = (int32_t)(x - s->node_off[g]);
            row.assign(in_idx.begin() + in_ptr[x], in_idx.begin() + in_ptr[x + 1]);
            row.insert(row.end(), out_idx.begin() + out_ptr[x], out_idx.begin() + out_ptr[x + 1]);
            std::sort(row.begin(), row.end());
            row.erase(std::unique(row.begin(), row.end()), row.end());
            for (const int32_t z : row)
                if (z != self) idx.push_back(z);
            ptr[x + 1] = (int64_t)idx.size();
            const int64_t d = ptr[x + 1] - ptr[x];
            deg[x] = (int32_t)d;
            aa[x] = d >= 2 ? (float)(1.0 / log((double)d)) : 0.f;
            ra[x] = d >= 1 ? (float)(1.0 / (double)d) : 0.f;
        }
        off[g + 1] = (int64_t)idx.size();
    }
    tm.lap("rows");
    int rc = nbr_upload(&s->d_nbr_ptr, ptr);
    if (rc == GM_OK) rc = nbr_upload(&s->d_nbr_idx, idx);
    if (rc == GM_OK) rc = nbr_upload(&s->d_nbr_deg, deg);
    if (rc == GM_OK) rc = nbr_upload(&s->d_nbr_aa, aa);
    if (rc == GM_OK) rc = nbr_upload(&s->d_nbr_ra, ra);
    // nothing of the upload is still on its way when the lock goes: a call on any stream may read the index from here on
    if (rc == GM_OK && hipStreamSynchronize(nullptr) != hipSuccess) { gm_set_error("neighbour index: upload failed"); rc = GM_EHIP; }
    if (rc != GM_OK) { nbr_release(s); return rc; }
    s->nbr_off = off;
    tm.lap("upload");
    return GM_OK;
}

int gm_nbr_index(const gm_store* s) {
    std::lock_guard<std::mutex> lk(s->nbr_mu);
    if (s->nbr_ready) return GM_OK;
    GM_TRY(nbr_build(s));
    s->nbr_ready = true;
    return GM_OK;
}

static int pair_graph_of(const gm_store* s, int32_t g, const char* what) {
    GM_REQUIRE(s, GM_EINVAL, "%s: store is NULL", what);
    GM_REQUIRE(g >= 0 && g < s->n_graphs, GM_EINVAL, "%s: graph %d of a store with %d graph(s)", what, g, s->n_graphs);
    return GM_OK;
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
    const int64_t no = s->node_off[g];
    const pair_graph G = {s->d_nbr_ptr + no, s->d_nbr_idx, s->d_nbr_aa + no, s->d_nbr_ra + no, s->node_off[g + 1] - no};
    const dim3 grid((unsigned)((n * lpp + GM_PAIR_THREADS - 1) / GM_PAIR_THREADS)), block(GM_PAIR_THREADS);      // n <= 2^31 - 1 pairs of at most 64 lanes: below 2^29 blocks
    if (lpp == 16) hipLaunchKernelGGL(k_pair_scores<16>, grid, block, 0, st, G, d_pairs, n, mask, d_out);
    else if (lpp == 32) hipLaunchKernelGGL(k_pair_scores<32>, grid, block, 0, st, G, d_pairs, n, mask, d_out);
    else hipLaunchKernelGGL(k_pair_scores<64>, grid, block, 0, st, G, d_pairs, n, mask, d_out);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

extern "C" int32_t gm_store_pair_scores(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, float* d_out, void* stream) {
    const char* what = "gm_store_pair_scores";
    GM_TRY(pair_graph_of(s, g, what));
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, GM_EINVAL, "%s: n = %lld", what, (long long)n);
    GM_REQUIRE((flags & ~GM_PAIR_MASK_TARGET) == 0, GM_EINVAL, "%s: unknown flag bits 0x%x (GM_PAIR_MASK_TARGET = 1)", what, (unsigned)flags);
    GM_TRY(gm_pair_lanes(s, g, what, nullptr));
    if (n == 0) return GM_OK;
    GM_REQUIRE(d_pairs && d_out, GM_EINVAL, "%s: NULL argument", what);
    GM_TRY(gm_nbr_index(s));
    int lpp = 0;
    GM_TRY(gm_pair_lanes(s, g, what, &lpp));                                             // (the library's choice reads the index's row lengths)
    return gm_pair_scores_launch(s, g, lpp, d_pairs, n, flags & GM_PAIR_MASK_TARGET, d_out, (hipStream_t)stream);
}

extern "C" int32_t gm_store_neighbour_degrees(const gm_store_t* s, int32_t g, int32_t* d_out, void* stream) {
    const char* what = "gm_store_neighbour_degrees";
    GM_TRY(pair_graph_of(s, g, what));
    GM_REQUIRE(d_out, GM_EINVAL, "%s: d_out is NULL", what);
    GM_TRY(gm_nbr_index(s));
    const int64_t no = s->node_off[g], N = s->node_off[g + 1] - no;
    GM_HIP(hipMemcpyAsync(d_out, s->d_nbr_deg + no, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GM_OK;
}
