// The neighbour index of a store: what the link-prediction calls read (pair_scores.hip, candidates.hip, pair_walks.hip, pair_pagerank.hip, pair_distance.hip; the kernels' side
// of it is gm_nbr.h) and gm_store_neighbour_degrees shows the degrees of.  The DEFINITION is in include/gmeta_hip.h.
//   the index   per node the ascending DISTINCT row of its in- and out-neighbours without itself (int64 row pointers over all graphs, int32 graph-local
//               ids) and deg, 1 / ln(deg), 1 / deg.  Built on the host at the first call that needs it: the in-rows of the store keep the caller's edge
//               order, so a merge needs a sort per row, and the build happens once per store.  It runs under gm_store::nbr_mu and the upload is complete on
//               the device before the lock is released, so every later call reads the index from whichever stream it runs on, with no event.
#include <math.h>
#include "gm_nbr.h"

void gm_nbr_release(const gm_store* s) {
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
    if (rc != GM_OK) { gm_nbr_release(s); return rc; }
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

gm_nbr_graph gm_nbr_graph_of(const gm_store* s, int32_t g) {
    const int64_t no = s->node_off[g];
    return {s->d_nbr_ptr + no, s->d_nbr_idx, s->node_off[g + 1] - no};
}

extern "C" int32_t gm_store_neighbour_degrees(const gm_store_t* s, int32_t g, int32_t* d_out, void* stream) {
    const char* what = "gm_store_neighbour_degrees";
    GM_TRY(gm_store_call_check(what, s, g));
    GM_REQUIRE(d_out, GM_EINVAL, "%s: d_out is NULL", what);
    GM_TRY(gm_nbr_index(s));
    const int64_t no = s->node_off[g], N = s->node_off[g + 1] - no;
    GM_HIP(hipMemcpyAsync(d_out, s->d_nbr_deg + no, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return GM_OK;
}
