// The gm_batch object between its build (extract.hip) and its consumers: slab allocator, stream ordering, destruction, the read-back exports.
// Host code only -- nothing here launches a kernel.
#include "gm_internal.h"

// Hop-label switch of the calling thread (gm_set_hop_labels): read where a batch is built
static thread_local int g_hop_labels = 0;
extern "C" void gm_set_hop_labels(int32_t D) {
    if (D < 0 || D > 7) { gm_set_error("gm_set_hop_labels: D=%d ignored (0 = off, 1..7 = label cap)", D); return; }
    g_hop_labels = D;
}
extern "C" int32_t gm_get_hop_labels(void) { return g_hop_labels; }
extern "C" int32_t gm_batch_hop_labels(const gm_batch_t* b) { return b ? b->hop_D : 0; }
void gm_batch_mark_use(const gm_batch* b, hipStream_t st) {
    if (!b || st == b->stream) return;              // same stream: the frees are already ordered behind the consumer
    if (!b->used_ev && hipEventCreateWithFlags(&b->used_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); b->used_ev = nullptr; return; }
    if (hipEventRecord(b->used_ev, st) != hipSuccess) (void)hipGetLastError();
}
int gm_batch_wait_build(const gm_batch* b, hipStream_t s) {
    if (s == b->stream) return GM_OK;
    hipEvent_t e;
    GM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); GM_HIP(hipEventRecord(e, b->stream)); GM_HIP(hipStreamWaitEvent(s, e, 0)); GM_HIP(hipEventDestroy(e));
    return GM_OK;
}

// Hub-part counters / partial rows of orientation o are about to be used by a launch on `s`: if the previous such launch went to ANOTHER
// stream, order this one behind everything queued there so far (which includes that launch).  Costs nothing while a batch stays on one stream.
int gm_batch_hub_order(const gm_batch* b, int o, hipStream_t s, int set) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    const int k = set * 2 + o;
    if (b->hub_used[k] && b->hub_stream[k] != s) {
        // The remembered stream may have been destroyed by its owner since: a failed record / wait must neither drop the ordering nor leave a
        // sticky error for the next hipGetLastError() -- fall back to draining the device before the scratch is reused.
        bool ordered = false;
        if (b->hub_ev[k] || hipEventCreateWithFlags(&b->hub_ev[k], hipEventDisableTiming) == hipSuccess)
            ordered = hipEventRecord(b->hub_ev[k], b->hub_stream[k]) == hipSuccess && hipStreamWaitEvent(s, b->hub_ev[k], 0) == hipSuccess;
        if (!ordered) {
            (void)hipGetLastError();
            GM_HIP(hipDeviceSynchronize());
        }
    }
    b->hub_used[k] = true; b->hub_stream[k] = s;
    return GM_OK;
}

// Second set of hub-part arrival counters and partial rows: the part tables are copied (device to device, on `s`, behind the batch's build),
// the counters start at zero like the first set's.
int gm_batch_hub_alt(const gm_batch* cb, hipStream_t s) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    gm_batch* b = const_cast<gm_batch*>(cb);
    bool waited = false;
    for (int o = 0; o < 2; ++o) {
        if (!b->d_hub[o] || b->d_hub2[o]) continue;
        int32_t* h2 = nullptr; float* sc2 = nullptr;
        GM_TRY(gm_balloc(b, &h2, (size_t)b->hub_words[o], b->stream));
        GM_TRY(gm_balloc(b, &sc2, (size_t)b->hub_parts[o] * GM_AGG_HUB_LD, b->stream));
        if (!waited && s != b->stream) { GM_TRY(gm_batch_wait_build(b, s)); waited = true; }
        GM_HIP(hipMemcpyAsync(h2, b->d_hub[o], sizeof(int32_t) * (size_t)b->hub_words[o], hipMemcpyDeviceToDevice, s));
        // (the first set's counters are zero between launches -- the last arriver resets them -- but a launch of the first set may be in flight on
        // another stream right now: zero the copy's counters explicitly)
        const size_t n_heavy = (size_t)b->n_heavy[o], parts = (size_t)b->hub_parts[o];
        GM_HIP(hipMemsetAsync(h2 + n_heavy + 1 + parts, 0, sizeof(int32_t) * n_heavy, s));
        b->d_hub2[o] = h2; b->d_hub_scratch2[o] = sc2;
    }
    if (waited) gm_batch_mark_use(b, s);
    return GM_OK;
}

int gm_balloc_bytes(gm_batch* b, void** p, size_t bytes, hipStream_t s) {
    std::lock_guard<std::mutex> lk(b->slab_mu);          // (lazily built tables -- receptive-field levels, stream tables, gains -- may come from another thread than the build's)
    bytes = (bytes + 255) / 256 * 256;
    if (b->slabs.empty() || b->slabs.back().cap - b->slabs.back().used < bytes) {
        // slab size: what the big arrays of this batch will need in total when the sizes are known (rows / edges; measured on the arxiv query batch:
        // 139 MB at 1.14 M rows / 2.1 M edges), plus room for the level arrays of a two-layer receptive-field build (12 + 4 bytes per row, 8 per edge:
        // cone.hip) so that a batch is ONE block of the slab cache; else 8 MiB steps
        const size_t guess = (size_t)b->rows * 78 + (size_t)b->edges * 31 + ((size_t)2 << 20) + (size_t)b->rows * 20 + (size_t)b->edges * 8 +
                             (b->hop_D ? (size_t)b->rows * (4 * (size_t)gm_pad_feat(gm_hop_feat_dim(b->store, b->centres, b->hop_D)) + 8) : 0);      // (+ a labelled batch's own feature table)
        gm_batch::slab sl{nullptr, 0, 0};
        GM_TRY(gm_slab_acquire(&sl.base, &sl.cap, std::max(bytes, b->slabs.empty() ? guess : std::max<size_t>(guess / 4, (size_t)8 << 20)), s));
        b->slabs.push_back(sl);
    }
    gm_batch::slab& sl = b->slabs.back();
    *p = sl.base + sl.used; sl.used += bytes;
    return GM_OK;
}

extern "C" void gm_batch_destroy(gm_batch_t* b) {
    if (!b) return;
    gm_phase_timer tm("batch-free");
    hipStream_t s = b->stream;
    for (int o = 0; o < 4; ++o) if (b->hub_ev[o]) { (void)hipEventDestroy(b->hub_ev[o]); b->hub_ev[o] = nullptr; }
    if (b->ro_ev) { (void)hipEventDestroy(b->ro_ev); b->ro_ev = nullptr; }
    if (b->used_ev) {
        if (hipStreamWaitEvent(s, b->used_ev, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipEventSynchronize(b->used_ev); }
        (void)hipEventDestroy(b->used_ev); b->used_ev = nullptr;
    }
    tm.lap("events");
    for (auto& sl : b->slabs) {      // every array of the batch lives in these (gm_balloc)
        gm_slab_release(sl.base, sl.cap, s);
        if (gm_knob().timing) { char nm[64]; snprintf(nm, sizeof nm, "slab %zu MB (%zu used)", sl.cap >> 20, sl.used >> 20); tm.lap(nm); }
    }
    b->slabs.clear();
    tm.lap("slabs");
    for (int l = 0; l <= GM_MAX_GCN; ++l) { gm_cone_free(b->cone[l], s); b->cone[l] = nullptr; }
    tm.lap("cones");
    delete b;
}

extern "C" int gm_batch_dims(const gm_batch_t* b, int64_t* rows, int64_t* edges, int32_t* subs, int32_t* sets, int32_t* centres) {
    GM_REQUIRE(b, GM_EINVAL, "batch_dims: NULL batch");
    if (rows) *rows = b->rows; if (edges) *edges = b->edges; if (subs) *subs = b->subs; if (sets) *sets = b->sets;
    if (centres) *centres = b->centres;
    return GM_OK;
}

static int field_ptr(const gm_batch_t* b, int32_t field, void** p, int64_t* bytes) {
    switch (field) {
        case GM_F_SUB_OFF: *p = b->d_sub_off; *bytes = 4ll * (b->subs + 1); break;
        case GM_F_SET_SUB_OFF: *p = b->d_set_sub_off; *bytes = 4ll * (b->sets + 1); break;
        case GM_F_PARENT: *p = b->d_parent; *bytes = 4ll * b->rows; break;
        case GM_F_GRAPH: *p = b->d_graph; *bytes = 4ll * b->subs; break;
        case GM_F_INDPTR: *p = b->d_indptr; *bytes = 4ll * (b->rows + 1); break;
        case GM_F_INDICES: *p = b->d_indices; *bytes = 4ll * b->edges; break;
        case GM_F_INDPTR_T: *p = b->d_indptr_t; *bytes = 4ll * (b->rows + 1); break;
        case GM_F_INDICES_T: *p = b->d_indices_t; *bytes = 4ll * b->edges; break;
        case GM_F_CENTRE: *p = b->d_centre; *bytes = 4ll * b->subs * b->centres; break;
        case GM_F_NORM: *p = b->d_norm; *bytes = 4ll * b->rows; break;
        case GM_F_FEAT_ROW: *p = b->d_store_row; *bytes = 4ll * b->rows; break;
        case GM_F_HOP:
            GM_REQUIRE(b->hop_D > 0, GM_EINVAL, "batch field GM_F_HOP: the batch carries no hop labels (built with gm_set_hop_labels(0))");
            *p = b->d_hop; *bytes = (int64_t)b->rows * b->centres; break;
        case GM_F_NORM_SRC: *p = b->d_norm_src; *bytes = 4ll * b->rows; break;
        case GM_F_NORM_CENTRE: *p = b->d_norm_c; *bytes = 4ll * b->rows; break;
        case GM_F_NORM_E1: *p = b->d_norm_e1; *bytes = 4ll * b->rows; break;
        case GM_F_EDGE_CENTRE_T: *p = b->d_ect; *bytes = 4ll * b->edges; break;
        case GM_F_OBS_CENTRE: *p = b->d_obs[0]; *bytes = 4ll * b->rows; break;
        case GM_F_OBS_E1: *p = b->d_obs[1]; *bytes = 4ll * b->rows; break;
        case GM_F_EDGE_W: case GM_F_EDGE_W_T:
            GM_REQUIRE(b->weighted, GM_EINVAL, "batch field %s: the batch is unweighted (its store was created without edge weights)", field == GM_F_EDGE_W ? "GM_F_EDGE_W" : "GM_F_EDGE_W_T");
            *p = b->d_ew[field == GM_F_EDGE_W ? 0 : 1]; *bytes = 4ll * b->edges; break;
        default: gm_set_error("unknown batch field %d", field); return GM_EINVAL;
    }
    return GM_OK;
}

extern "C" int gm_batch_read(const gm_batch_t* b, int32_t field, void* host_dst, int64_t bytes) {
    GM_REQUIRE(b && host_dst, GM_EINVAL, "batch_read: NULL argument");
    void* p; int64_t need;
    GM_TRY(field_ptr(b, field, &p, &need));
    GM_REQUIRE(bytes >= need, GM_EINVAL, "batch_read: destination holds %lld bytes, field needs %lld", (long long)bytes, (long long)need);
    if (field == GM_F_CENTRE && (int64_t)b->h_centre.size() * 4 == need) { memcpy(host_dst, b->h_centre.data(), (size_t)need); return GM_OK; }
    GM_HIP(hipMemcpyAsync(host_dst, p, (size_t)need, hipMemcpyDeviceToHost, b->stream));
    GM_HIP(hipStreamSynchronize(b->stream));
    return GM_OK;
}

extern "C" int32_t gm_batch_weighted(const gm_batch_t* b) { return b && b->weighted ? 1 : 0; }
extern "C" int32_t gm_batch_mask_target(const gm_batch_t* b) { return b && b->mask_target ? 1 : 0; }
extern "C" int gm_batch_source_rows(const gm_batch_t* b, int64_t* n_rows) {
    GM_REQUIRE(b && n_rows, GM_EINVAL, "batch_source_rows: NULL argument");
    *n_rows = b->n_src;
    return GM_OK;
}
extern "C" int gm_batch_e1_source_rows(const gm_batch_t* b, int64_t* n_rows) {
    GM_REQUIRE(b && n_rows, GM_EINVAL, "batch_e1_source_rows: NULL argument");
    *n_rows = gm_batch_e1_rows(b, b->stream);
    return GM_OK;
}
extern "C" int gm_batch_device_ptr(const gm_batch_t* b, int32_t field, void** dptr) {
    GM_REQUIRE(b && dptr, GM_EINVAL, "batch_device_ptr: NULL argument");
    int64_t bytes;
    return field_ptr(b, field, dptr, &bytes);
}
