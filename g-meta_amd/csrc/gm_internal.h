// Internal declarations shared by the HIP translation units of libgmeta_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include "gm_bound.h"
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../../include/gmeta_hip.h"

#define GM_WAVE 64
#define GM_NXCD 8

void gm_set_error(const char* fmt, ...);

#define GM_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            gm_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return GM_EHIP;                                                                       \
        }                                                                                         \
    } while (0)
#define GM_REQUIRE(cond, code, ...)  \
    do {                             \
        if (!(cond)) {               \
            gm_set_error(__VA_ARGS__); \
            return (code);           \
        }                            \
    } while (0)
#define GM_TRY(call)            \
    do {                        \
        int r__ = (call);       \
        if (r__ != GM_OK) return r__; \
    } while (0)

struct gm_store {
    int32_t n_graphs = 0, feat_dim = 0;
    int32_t feat_ld = 0;             // row stride of d_feat: feat_dim padded with zero columns (32, else a multiple of 64) so that layer 1 runs on the
                                     // vectorised aggregate / DMA GEMM / fast weight-gradient kernels whatever the dataset's feature width
    int64_t total_nodes = 0, total_edges = 0, max_nodes = 0;
    std::vector<int64_t> node_off, edge_off;      // host prefix sums per graph
    // device
    int64_t* d_node_off = nullptr;   // [G+1]
    int64_t* d_in_ptr = nullptr;     // [total_nodes + 1] global edge offsets, rows = global node ids
    int32_t* d_in_idx = nullptr;     // [total_edges]     source node, LOCAL to its graph
    int64_t* d_out_ptr = nullptr;    // by-source CSR of the same edges (for the transposed induce)
    int32_t* d_out_idx = nullptr;    // destination node, LOCAL to its graph
    bool symmetric = false;          // out-CSR == in-CSR element for element (extract.hip: adjacency lists walked once)
    bool weighted = false;           // created with edge weights (gm_store_create_weighted): every batch cut from it carries them
    float* d_in_w = nullptr;         // [total_edges] weight of the edge, aligned with d_in_idx (weighted stores only)
    float* d_out_w = nullptr;        // ... aligned with d_out_idx
    float* d_feat = nullptr;         // [total_nodes, feat_ld]
    unsigned* d_feat_amax = nullptr; // [1] bit pattern of max |feature| over the whole table
    // per graph (host): max |x| and mean |x| over the non-zero entries.  The two-piece fp16 kernels (opt-in, gm_bound.h) bound the layer-1 operand
    // of a task by the largest feature of the graphs the task draws from, and keep the three-piece kernels for a pass whose table is LOOSE: an
    // entry 2^r below its bound keeps min(22, 39 - r) bits, so a table whose largest entry sits more than 2^14 above its typical one (or is
    // not finite / above 2^50) would lose precision silently
    std::vector<float> h_feat_amax, h_feat_mean;
    // neighbour index of the link-prediction calls (nbr_index.hip; what the kernels see of it: gm_nbr.h; definition: include/gmeta_hip.h): per node the ascending DISTINCT row of its in- and out-neighbours
    // without itself, and the per-node terms.  Built at the first call that needs it, under nbr_mu, and complete on the device before nbr_ready is set:
    // afterwards any stream reads it without an event.  Freed by gm_store_destroy.
    mutable std::mutex nbr_mu;
    mutable bool nbr_ready = false;
    mutable int64_t* d_nbr_ptr = nullptr;     // [total_nodes + 1] offsets into d_nbr_idx, rows = global node ids
    mutable int32_t* d_nbr_idx = nullptr;     // [<= 2 total_edges] neighbour, LOCAL to its graph, ascending inside a row
    mutable int32_t* d_nbr_deg = nullptr;     // [total_nodes] deg = row length
    mutable float* d_nbr_aa = nullptr;        // [total_nodes] 1 / ln(deg), deg >= 2, else 0
    mutable float* d_nbr_ra = nullptr;        // [total_nodes] 1 / deg, deg >= 1, else 0
    mutable std::vector<int64_t> nbr_off;     // [n_graphs + 1] host prefix of the row lengths per graph (mean distinct degree -> lanes per pair)
};

// Receptive-field tables (cone.hip): level l = rows whose layer-l activation reaches a centre.
struct gm_cone_level {
    int32_t n = 0, nnz = 0;            // rows of this level; edges from level l-1 into it
    int32_t* d_row = nullptr;          // [n]  batch row (ascending; level L: centre order)
    float* d_norm = nullptr;           // [n]  norm[row]
    int32_t* d_feat_row = nullptr;     // level 0 only: [n] feature row in the store
    int32_t* d_set_off = nullptr;      // [sets+1] compact row range of every set
    std::vector<int32_t> h_set_off;
    int32_t* d_tiles = nullptr; int32_t n_tiles = 0;                 // GEMM row tiles over the compact rows
    int32_t* d_chunks = nullptr; int32_t* d_set_chunk_off = nullptr; int32_t n_chunks = 0;
    int32_t* d_indptr = nullptr; int32_t* d_indices = nullptr;       // [n+1], [nnz]: in-edges, sources = compact ids of level l-1
    int32_t* d_indptr_t = nullptr; int32_t* d_indices_t = nullptr;   // [n_{l-1}+1], [nnz]: the same edges by source, destinations = compact ids of level l
    // weighted batches only (NULL otherwise), per edge: its weight and weight x norm of the row the aggregate reads -- aligned with d_indices (source = level l-1)
    // and with d_indices_t (source = level l); level 1 also the feature row of the edge's source, what its weighted gather needs beside the coefficient
    float* d_ew = nullptr; float* d_enorm = nullptr; float* d_ew_t = nullptr; float* d_enorm_t = nullptr; int32_t* d_efeat = nullptr;
    int32_t* d_heavy[2] = {nullptr, nullptr}; int32_t n_heavy[2] = {0, 0};
};
struct gm_cone {
    int L = 0; bool ok = false; int heavy_deg = 64;
    gm_cone_level lv[GM_MAX_GCN + 1];
    void* slab = nullptr;           // every device array of the levels is carved from this one region of the BATCH's slabs (sized from upper bounds: cone.hip); released with the batch
};
struct gm_batch;
int gm_batch_cone(const gm_batch* b, int L, hipStream_t s, const gm_cone** out);   // built on first use, cached in the batch
void gm_cone_free(gm_cone* c, hipStream_t s);

struct gm_batch {
    const gm_store* store = nullptr;
    int64_t rows = 0, edges = 0;
    int32_t subs = 0, sets = 0, centres = 1;
    // host mirrors (small)
    std::vector<int32_t> h_sub_off, h_set_sub_off, h_set_row_off, h_graph;
    // device
    int32_t* d_sub_off = nullptr;      // [subs+1]
    int32_t* d_set_sub_off = nullptr;  // [sets+1]
    int32_t* d_set_row_off = nullptr;  // [sets+1]
    int32_t* d_graph = nullptr;        // [subs]
    int32_t* d_parent = nullptr;       // [rows]
    int32_t* d_feat_row = nullptr;     // [rows]  row of the feature table below (labelled batches: the identity)
    // The feature table layer 1 gathers from: the store's (default), or -- hop-labelled batches, gm_set_hop_labels -- the batch's own
    // [rows, feat_ld] table of store features + one-hot label columns + zero padding (k_label_features).  Every gather path reads these four.
    const float* feat = nullptr; int64_t feat_ld = 0, feat_rows = 0; int32_t feat_dim = 0;
    int32_t hop_D = 0;                 // label cap D of a labelled batch (0: unlabelled)
    int8_t* d_hop = nullptr;           // [rows, centres] hop-distance labels (GM_F_HOP; labelled batches only)
    int32_t* d_store_row = nullptr;    // [rows]  row of the STORE's feature matrix (GM_F_FEAT_ROW): d_feat_row itself on unlabelled batches
    int32_t* d_indptr = nullptr;       // [rows+1]
    int32_t* d_indices = nullptr;      // [edges]
    int32_t* d_indptr_t = nullptr;     // [rows+1]
    int32_t* d_indices_t = nullptr;    // [edges]
    int32_t* d_centre = nullptr;       // [subs*centres] local index
    std::vector<int32_t> h_centre;     // host copy, brought by the finalisation's round trip (gm_batch_read serves it without another one)
    float* d_norm = nullptr;           // [rows]
    bool weighted = false;             // cut from a weighted store: d_ew holds the induced edge weights, d_norm the weighted in-degree's norm
    bool mask_target = false;          // built with GM_LINK_MASK_TARGET: the CSR (and everything derived from it) holds no edge between a subgraph's two centres
    float* d_ew[2] = {nullptr, nullptr};   // [edges] weight of every edge, aligned with d_indices / d_indices_t (weighted batches only)
    // derived launch tables (built by gm_batch_finalize)
    int32_t* d_sub_set = nullptr;      // [subs]  set of each subgraph
    int32_t* d_tiles = nullptr;        // [n_tiles*3]  GEMM row tiles: set, row0, nrows (<= GM_GEMM_BM)
    int32_t n_tiles = 0;
    int32_t* d_chunks = nullptr;       // [n_chunks*3] weight-gradient row chunks: set, row0, nrows
    int32_t n_chunks = 0;
    int32_t* d_set_chunk_off = nullptr;// [sets+1]
    int32_t* d_heavy[2] = {nullptr, nullptr};   // rows with more than gm_heavy_deg() edges, by-destination / by-source CSR
    int32_t n_heavy[2] = {0, 0};
    int32_t heavy_deg = 64;
    // block schedule of the window aggregate (one launch: hub-row blocks are interleaved with the window blocks of their
    // own subgraph on the XCD that owns them, see gm_agg_schedule): [8 * sched_len] entries per orientation
    int32_t* d_sched[2] = {nullptr, nullptr};
    int32_t sched_len[2] = {0, 0};
    int32_t sched_win = 0;
    // hub rows split into parts of hub_part edges, one block each (gm_agg_schedule): part table + arrival counters, and the partial
    // rows.  One aggregate launch per orientation at a time (a batch's launches are stream-ordered: they share the layer buffers too).
    int32_t* d_hub[2] = {nullptr, nullptr}; float* d_hub_scratch[2] = {nullptr, nullptr}; int32_t hub_part[2] = {0, 0};
    int32_t hub_words[2] = {0, 0}, hub_parts[2] = {0, 0};      // size of d_hub[o] (int32 words) and its part count (d_hub_scratch[o]: parts x GM_AGG_HUB_LD floats)
    // a SECOND set of arrival counters / partial rows (gm_batch_hub_alt): lets two streams run aggregate launches over the batch at the same
    // time (gm_meta_step's two query streams); the part tables are copies, only the counters and the partial rows are private
    mutable int32_t* d_hub2[2] = {nullptr, nullptr}; mutable float* d_hub_scratch2[2] = {nullptr, nullptr};
    // The arrival counters / partial rows belong to ONE launch at a time.  Launches of a batch are stream-ordered in gm_meta_step; a caller
    // that moves an orientation's launches to another stream (public gm_aggregate / gm_gcn_* API) is ordered behind the previous stream's
    // launch by gm_batch_hub_order (an event wait, only when the stream changes).  Host-side bookkeeping, guarded by hub_mu.
    mutable hipStream_t hub_stream[4] = {nullptr, nullptr, nullptr, nullptr}; mutable bool hub_used[4] = {false, false, false, false}; mutable hipEvent_t hub_ev[4] = {nullptr, nullptr, nullptr, nullptr};      // [set * 2 + orientation]
    // per-edge tables (gm_batch_finalize): the source's norm for both CSR orientations (enorm[o][e] = norm[indices_o[e]]; weighted batches:
    // d_ew[o][e] * norm[indices_o[e]] -- this table and d_fuse2's w0 / w1 are where the weights meet the model's kernels) and the source's
    // feature row (efeat[e] = feat_row[indices[e]]): what the aggregate would otherwise fetch with a dependent 4-byte gather per edge
    float* d_enorm[2] = {nullptr, nullptr}; int32_t* d_efeat = nullptr;
    // row gains of the two aggregates (gm_bound.h): |out| <= gain * max |in| -- [0] forward: max_i sum_{u->i} norm[u]; [1] transposed with the
    // destination's norm on the output (the backward of an aggregate-first layer): max_i norm[i] * outdeg(i)
    float* d_gain = nullptr;
    // fused aggregate + GEMM (forward passes nobody differentiates): per row {u0, u1, bits(w0), bits(w1)} -- the row's one or two sources
    // (batch rows in d_fuse2, feature rows in d_fuse2_feat) and their norms; rows without a source carry {GM_FUSE_ZERO, same, 1, 0}, rows of any other degree {row | GM_FUSE_SELF, same, 1, 0}:
    // their aggregate is written by the ordinary kernel (gm_agg_args::skip_lo/hi) and picked up as is
    void* d_fuse2 = nullptr; void* d_fuse2_feat = nullptr;
    int64_t unfused_rows = 0, unfused_edges = 0;     // rows (and their in-edges) the ordinary aggregate still writes in a fused pass
    // The partial aggregate launch of a fused pass walks a COMPACT list of its window rows (in-degree GM_FUSE_MAXDEG+1 .. heavy_deg, ascending)
    // instead of every row of the batch: 8 % of the rows of the arxiv query batch carry work in that launch, and a wave whose 16-row window holds
    // one of them runs its gathers one dependent batch at a time; with the list every wave window is full of rows that have work.
    int32_t* d_mid = nullptr; int32_t n_mid = 0, mid_win = 0;
    // stream aggregate (agg_stream.hip), per orientation: row bounds in the stream edge tables (hub rows hold no edges in the row-ordered part; bit 31 of a
    // hub row's end bound flags it), the per-edge source / weight tables in row order with the hub rows' edges behind (d_su_feat: sources = feature rows
    // of the store, layer 1), the prefix of the hub rows' edge counts, the cost-balanced row segments of the launch's waves and its grid split
    int32_t* d_sptr[2] = {nullptr, nullptr}; int32_t* d_su[2] = {nullptr, nullptr}; int32_t* d_su_feat = nullptr; float* d_sw[2] = {nullptr, nullptr};
    int32_t* d_scum[2] = {nullptr, nullptr}; int2* d_sseg[2] = {nullptr, nullptr}; int32_t* d_sxord[2] = {nullptr, nullptr};
    int32_t stream_nseg[2] = {0, 0}, stream_nwg[2] = {0, 0}, stream_hubwg[2] = {0, 0}, stream_nparts[2] = {0, 0}, stream_enorm[2] = {0, 0};
    // The stream tables are built at the FIRST launch that can take the stream kernel (gm_agg_stream_args; round 6), from what the finalisation's round trip
    // brought to the host: with the fused passes of the dense schedule only a large support batch ever gets there, and never the by-source orientation --
    // built with every batch they were 0.23 ms of host time and eight kernels of each 32-task query batch for nothing.
    struct stream_pending { bool pending = false; bool has_tab = false; int n_parts = 0; std::vector<int32_t> hubs, deg, tab; };
    mutable stream_pending spend[2];
    int32_t* d_sched_mid = nullptr; int32_t sched_len_mid = 0;      // block schedule over the list (hub parts placed by the hub row's approximate list position)
    mutable int64_t unfused_src = -1;                // DISTINCT source rows of those in-edges (profiling only: counted on first use, gm_batch_unfused_sources)
    // compact row lists for the row-sparse backward (gm_hparams_t.sparse_bwd)
    int32_t n_c = 0;                   // centre rows: subs * centres
    int32_t* d_crow = nullptr;         // [n_c]  batch row of every centre
    float* d_cnorm = nullptr;          // [n_c]  norm[centre row]
    float* d_norm_c = nullptr;         // [rows] norm with the SIGN BIT SET on every row that is not a centre: row scale + "somebody reads this row" flag of the last layer's
                                       //        forward-only update (gm_gemm_args::row_scale_keep)
    // GM_DEAD_ROWS (k_row_tables, same pass): the same flag for the layers BELOW the last, whose activations are read through the edges only --
    float* d_norm_src = nullptr;       // [rows] norm with the SIGN BIT SET on every row without an out-edge inside the batch (nobody's source: H_l of that row has no reader)
    int64_t n_src = 0;                 //        rows WITH an out-edge (the rows those updates store)
    void* d_dq_tab = nullptr;          // [rows] int4, laid out like d_fuse2: centre rows {row | GM_FUSE_SELF, GM_FUSE_ZERO, 1, 0}, every other row {GM_FUSE_ZERO, GM_FUSE_ZERO, 0, 0} --
                                       //        the dZ GEMM of the last layer reads dQ_L through it (only its centre rows were ever written)
    int32_t n_e1 = 0;                 // in-edges of centres, concatenated in centre order
    int32_t* d_e1_row = nullptr;       // [n_e1] source row of the edge
    int32_t* d_e1_par = nullptr;       // [n_e1] compact index of the centre it enters
    // GM_DEAD_ROWS=2 (k_e1_tables / k_e1_rows, after k_centre_edges): one level below d_norm_c / d_dq_tab.  T = norm (dQ_L W_L^T) is zero outside the centre rows, and
    // dQ_{L-1} = relu' norm A^T T outside the sources of the centres' in-edges
    int32_t* d_ect = nullptr;          // [edges] source row of T for every edge of the by-source CSR: indices_t[e] where that row is a centre, else a row of the zero
                                       //        block behind T (rows + (e & (GM_ZERO_ROWS - 1))): gm_agg_args::x_idx of the last layer's transposed aggregate
    float* d_norm_e1 = nullptr;        // [rows] norm with the SIGN BIT SET on every row that is not the source of an in-edge of a centre (gm_agg_args::s_out + keep_signed of that
                                       //        launch, gm_wgrad_args::g_keep of the weight gradient below it)
    int32_t* d_n_e1_rows = nullptr;    // [1]    rows with the bit clear, counted on the device (gm_batch_e1_rows reads it at first use)
    mutable int64_t n_e1_rows = -1;
    mutable int64_t n_e1_edges = -1;   //        by-source edges of those rows (profiling only: counted on first use, gm_batch_e1_edges)
    // GM_DEAD_ROWS=3 (k_fwd_tables, after k_e1_rows): the same two row sets for the passes nobody differentiates, whose only observable values are the centre rows
    // of H_L.  [0]: the last layer (observable rows = the centre rows), [1]: the layer below it (the sources of the centres' in-edges)
    void* d_fwd_tab[2] = {nullptr, nullptr};   // [rows] int4: d_fuse2's entry on the observable rows, {GM_FUSE_ZERO, GM_FUSE_ZERO, 0, 0} on every other row (gm_gemm_args::fuse2)
    void* d_fwd_tab_feat = nullptr;            // [rows] int4: d_fuse2_feat's entry on the [1] rows -- where the layer below the last gathers from the feature table
    float* d_obs[2] = {nullptr, nullptr};      // [rows] +1 on the observable rows, -1 on every other row: gm_agg_args::s_out + keep_signed of the partial aggregate launches (a scale of exactly 1)
    // GM_DEAD_TILES (k_tile_live, next to k_fwd_tables): one word per tile of d_tiles, non-zero where some row of the tile has the sign bit of d_norm_c ([0]) / d_norm_e1 ([1])
    // clear.  A split GEMM that stores those rows only issues a zero tile's MFMAs and nothing else of it (gm_gemm_args::tile_live)
    int32_t* d_tile_live[2] = {nullptr, nullptr};
    // GM_PACK_ROWS (k_pack_rows / k_pack_tiles, at the end of the finalisation): the same two row sets PACKED per set (task), ascending by row, into the fewest tiles --
    // [0] the rows with the sign of d_norm_c clear, [1] those of d_norm_e1.  Set t owns entries [base_t, base_t + kept_t) of the packed arrays, base_t the prefix of the
    // host's bounds (the set's centres / the in-edges of its centres, capped by its rows).  rowid: batch row of every packed entry; scale: |keep vector| of that row;
    // tab[k]: src_tab[k]'s entry of that row (centres: d_fwd_tab[0], d_dq_tab; e1: d_fwd_tab[1], d_fwd_tab_feat); tiles: {set, offset, nrows <= GM_GEMM_BM} in d_tiles'
    // format, *count of them (a set without a kept row has none; never more than cap_tiles, and never more than the set's own tiles of d_tiles).
    // A split GEMM that would take d_tile_live feeds these tiles instead and stores row r of a tile at rowid[offset + r] (gm_gemm_args::pack)
    struct pack_set { int32_t* rowid = nullptr; int32_t* tiles = nullptr; int32_t* count = nullptr; float* scale = nullptr; const float* keep = nullptr;
                      const void* src_tab[2] = {nullptr, nullptr}; void* tab[2] = {nullptr, nullptr}; int32_t* set_cnt = nullptr; int32_t cap_rows = 0, cap_tiles = 0; };
    pack_set pack[2];
    // The observable rows of the restricted aggregate launches as compact ascending lists (finalize_finish, next to d_mid; GM_AGG_OBS_LIST).  [0]: rows of GM_FUSE_MAXDEG+1 ..
    // heavy_deg in-edges with d_obs[0] positive (the last layer's partial aggregate), [1]: the same with d_obs[1] (the layer below), [2]: rows with the sign of d_norm_e1
    // clear (the last layer's transposed aggregate; its hub rows stay listed, the windows pass over them).  [0] is built on the host from the centres' in-degrees (length
    // exact, len == NULL); [1] / [2] by the d_mid compaction with the flag as a second condition: cap is the host's bound (min(n_e1, rows walked today)), it sizes list,
    // grid and schedule, and the launch reads the true length from *len (gm_agg_args::n_list_dev).  take: 0 today's launch (no list: bound not below half the rows walked
    // today, hub tables missing), 1 the list, 2 nothing to launch (known on the host: no row of the set has work).  sched: block schedule over the list where the orientation has hub rows
    struct obs_list { int32_t* rows = nullptr; int32_t* len = nullptr; int32_t cap = 0, win = 0, take = 0; int32_t* sched = nullptr; int32_t sched_len = 0; mutable int64_t n = -1; };
    obs_list obs[3];
    mutable int64_t fwd_cnt[2][3] = {{-1, -1, -1}, {-1, -1, -1}};      // observable rows of more than GM_FUSE_MAXDEG sources, their in-edges, their distinct sources (profiling only: counted on first use, gm_batch_fwd_counts)
    float* d_e1_norm = nullptr;        // [n_e1] norm[source row]
    float* d_e1_coef = nullptr;        // [n_e1] weighted batches only: edge weight x norm[source row] (the transposed aggregate's coefficient; d_e1_norm stays the row scale)
    int32_t* d_c_tiles = nullptr; int32_t n_c_tiles = 0;          // GEMM tiles over centre rows (per set)
    int32_t* d_c_chunks = nullptr; int32_t* d_c_set_chunk_off = nullptr; int32_t n_c_chunks = 0;
    int32_t* d_e1_chunks = nullptr; int32_t* d_e1_set_chunk_off = nullptr; int32_t n_e1_chunks = 0;
    // mean readout (gm_set_readout; model.hip: readout_tables), built at first use from h_sub_off: every subgraph cut into chunks of GM_RO_ROWS rows, one int4
    // {row0, rows, subgraph, rows of the subgraph} per chunk, and one int4 {subgraph, first chunk, chunks, rows} per subgraph of more than one chunk
    mutable int32_t* d_ro_chunks = nullptr; mutable int32_t* d_ro_multi = nullptr; mutable int32_t n_ro_chunks = 0, n_ro_multi = 0;
    // the upload went to ro_stream and ro_ev was recorded behind it: a later caller on ANOTHER stream waits on it before its kernels read the tables
    mutable hipStream_t ro_stream = nullptr; mutable hipEvent_t ro_ev = nullptr;
    mutable gm_cone* cone[GM_MAX_GCN + 1] = {};     // receptive-field tables per number of GCN layers (gm_hparams_t.cone)
    hipStream_t stream = nullptr;      // stream the arrays were produced on (and are freed on, stream-ordered)
    // The ~45 device arrays above are carved out of a few slabs (gm_balloc): a stream-ordered allocation or free costs the host 20-35 us, and a
    // meta-batch builds and drops two batches per step (3 ms of frees in Subgraphs.get_batch before this)
    struct slab { char* base; size_t cap, used; };
    std::vector<slab> slabs;
    std::mutex slab_mu;
    mutable hipEvent_t used_ev = nullptr;   // last consumer on ANOTHER stream: the frees wait for it (gm_batch_mark_use)
};
int gm_batch_gains(const gm_batch* b, hipStream_t s);
// n elements of T from the batch's slabs (256-byte aligned; lives until the batch is destroyed)
int gm_balloc_bytes(gm_batch* b, void** p, size_t bytes, hipStream_t s);
template <class T> static inline int gm_balloc(gm_batch* b, T** p, size_t n, hipStream_t s) { return gm_balloc_bytes(b, (void**)p, (n ? n : 1) * sizeof(T), s); }     // d_gain at first use (two-piece kernels only)
// A consumer that ran kernels over the batch on `st` calls this afterwards: gm_batch_destroy then orders its frees behind
// that work instead of relying on the host having synchronised (deferred read-back, prefetch threads).
void gm_batch_mark_use(const gm_batch* b, hipStream_t st);
int gm_batch_wait_build(const gm_batch* b, hipStream_t s);      // orders s behind everything queued on the batch's build stream so far (nothing when s is that stream)
// feature width of a batch labelled with cap D (gm_set_hop_labels): D + 2 one-hot columns per centre behind the store's features
static inline int gm_hop_feat_dim(const gm_store* st, int centres, int D) { return st->feat_dim + centres * (D + 2); }

// ---- tuning / debug knobs: every GM_* environment variable is read ONCE, under std::call_once, into this
// struct (the prefetch thread and the training thread both enter the library); per-device quantities are derived at the call site.
struct gm_knobs {
    int timing;
    int extract_pref16;            // GM_EXTRACT_PREF16: 16-bit per-word prefix counts in the extraction kernels' LDS (1, default): four resident workgroups per CU instead of three at the arxiv parent size
    int gemm_mode;                 // 0 exact fp32, 1 split-bf16, -1 not set (library default)
    int gemm_split_min_tiles;      // -1: a quarter of the current device's CUs
    // GM_CENTRE_STORE (0..2, default 2), GM_DEAD_ROWS (0..4, default 4), GM_FUSE_DIFF (0..2, default 2): which rows a pass of the dense schedule forms, stores and
    // zero-fills, and which of its layers run fused.  What each value means and how the three combine: the table in DESIGN.md section 4.3; read by plan_pass (model.hip) alone
    int centre_store, dead_rows;
    int fuse_agg, head_stage;
    int fuse_diff;
    int agg_mid_win;               // GM_AGG_MID_WIN: rows per wave window over that list (0 = by its length)
    int agg_obs_list;              // GM_AGG_OBS_LIST: the aggregate launches restricted to the observable rows walk the batch's compact lists of them (1, default; gm_batch::obs) or every row's descriptor (0).  Read at launch time (plan_pass): the lists are built either way
    int dead_tiles;                // GM_DEAD_TILES: a fused three-piece split GEMM that stores the rows of a keep vector only takes the batch's tile flags (1, default; gm_batch::d_tile_live): a tile without a kept row issues its MFMAs on zero registers and nothing else.  0: every tile is fed.  Read by plan_pass alone; the flags are built either way
    int pack_rows;                 // GM_PACK_ROWS: a launch that takes the tile flags takes the row set's packed tiles instead (1, default; gm_batch::pack): the kept rows fill the fewest tiles, every other tile is a dead one.  0: the tile flags.  Read by plan_pass alone; the tables are built either way
    int agg_mid_list;              // GM_AGG_MID_LIST: the partial aggregate launch of a fused pass walks a compact list of its window rows (1, default) or every row (0)
    int query_streams;             // GM_QUERY_STREAMS: 2 = the query evaluations of gm_meta_step alternate between two streams; anything else (default 0) = one stream
    int head_threads;              // GM_HEAD_THREADS: workgroup size of k_head_loss: 256 or 512; anything else (default 0) = 1024
    int split16_min_rows;          // GM_SPLIT16_MIN_ROWS: support + query rows from which gm_meta_step takes the two-piece kernels (smaller steps are launch-bound: no gain)
    int split_pieces;              // GM_SPLIT_PIECES: pieces per operand of the split kernels inside gm_meta_step: 3 = exact bf16 triple, all 24 operand bits (default); 2 = opt-in fp16 pair under recorded bounds
    int wgrad_split_min_chunks;    // GM_WGRAD_SPLIT_MIN_CHUNKS: smallest launch (row chunks) that takes the split weight-gradient kernel; -1: a quarter of the CUs
    int agg_stream;                // GM_AGG_STREAM: eligible full aggregate launches take the LDS-DMA stream kernel (agg_stream.hip)
    int agg_stream_min_rows;       // GM_AGG_STREAM_MIN_ROWS: smallest batch (rows) that builds stream tables; dense batches (more than 8 edges per row) never do
    int neg_round;                 // GM_NEG_ROUND, gm_set_tuning("neg_round"): candidates per round of gm_store_negative_pairs (negatives.hip); 0 (default) = by the call's n.  The result does not depend on it
    int pair_lanes;                // GM_PAIR_LANES, gm_set_tuning("pair_lanes"): lanes per pair of gm_store_pair_scores (pair_scores.hip): 16, 32 or 64; 0 (default) = by the graph's mean distinct degree
    int cand_round;                // GM_CAND_ROUND, gm_set_tuning("cand_round"): pairs per round of gm_store_pair_candidates (candidates.hip); 0 (default) = the library's choice.  The result does not depend on it
    int walk_chunk;                // GM_WALK_CHUNK, gm_set_tuning("walk_chunk"): outer-row entries per work item of gm_store_pair_walks (pair_walks.hip); 0 (default) = the library's choice.  The result does not depend on it
    int walk_lanes;                // GM_WALK_LANES, gm_set_tuning("walk_lanes"): lanes per work item of gm_store_pair_walks: 32 or 64; 0 (default) = by the graph's mean distinct degree and the length of the pair list.  The result does not depend on it
    int ppr_chunk;                 // GM_PPR_CHUNK, gm_set_tuning("ppr_chunk"): entries per segment of a hub row of gm_store_rooted_pagerank / gm_store_pair_pagerank (pair_pagerank.hip); 0 (default) = the library's choice.  The order of a row sum, hence the low bits of the result, belongs to it
    int ppr_cols;                  // GM_PPR_COLS, gm_set_tuning("ppr_cols"): columns per round of those two calls, a multiple of 64; 0 (default) = the library's choice.  The result does not depend on it
    int dist_chunk;                // GM_DIST_CHUNK, gm_set_tuning("dist_chunk"): entries per segment of a hub row of gm_store_node_distances / gm_store_pair_distance (pair_distance.hip); 0 (default) = the library's choice.  The result does not depend on it
    int dist_cols;                 // GM_DIST_COLS, gm_set_tuning("dist_cols"): columns per round of those two calls, a multiple of 64 up to 4096; 0 (default) = the library's choice.  The result does not depend on it
    int dist_plane_kib;            // GM_DIST_PLANE_KIB, gm_set_tuning("dist_plane_kib"): KiB of level planes gm_store_pair_distance_profile may hold at a time (pair_distance.hip), which bounds the columns of a group; 0 (default) = the library's choice, 1 GiB.  The result does not depend on it
    int cand_bitmap;               // GM_CAND_BITMAP, gm_set_tuning("cand_bitmap"): home of that call's membership bitmap: 1 LDS, 2 a per-workgroup slab in HBM; 0 (default) = LDS wherever the graph fits.  The result does not depend on it
    int sketch_chunk;              // GM_SKETCH_CHUNK, gm_set_tuning("sketch_chunk"): entries per segment of a hub row of gm_store_sketch_build (node_sketches.hip); 0 (default) = the library's choice.  The result does not depend on it
    int sketch_mib;                // GM_SKETCH_MIB, gm_set_tuning("sketch_mib"): MiB one gm_store_sketch_build may allocate; 0 (default) = the library's choice, 8 GiB.  The result does not depend on it
    int prop_chunk;                // GM_PROP_CHUNK, gm_set_tuning("prop_chunk"): entries per segment of a hub row of gm_store_propagate_build (propagate.hip); 0 (default) = the library's choice.  The order of a row's fp32 sum, hence its low bits, belongs to it
    int prop_mib;                  // GM_PROP_MIB, gm_set_tuning("prop_mib"): MiB one gm_store_propagate_build may allocate; 0 (default) = the library's choice, 8 GiB.  The result does not depend on it
    int pair_mlp_rows;             // GM_PAIR_MLP_ROWS, gm_set_tuning("pair_mlp_rows"): pairs per chunk of gm_prop_pair_mlp_step (pair_mlp.hip), which bounds its dh scratch; 0 (default) = the library's choice.  The logits do not depend on it; the summation order of the loss and the gradients, hence their low bits, belongs to it
    int rank_sort_min;             // GM_RANK_SORT_MIN, gm_set_tuning("rank_sort_min"): the N at or above which the shared mode of gm_rank_counts / gm_rank_summary (ranking.hip) sorts the negatives instead of sweeping them; 0 (default) = the library's choice, 1 = always, INT32_MAX = never.  The result does not depend on it
};
const gm_knobs& gm_knob();

// ---- the hop-propagated features of one graph (propagate.hip builds and reads them; pair_mlp.hip gathers their rows into its GEMMs)
struct gm_prop {
    int64_t N = 0, bytes = 0;
    int32_t hops = 0, F = 0, ld = 0, flags = 0;
    float* d = nullptr;                   // [hops + 1][N][ld]
};

// ---- the neighbour index (nbr_index.hip; the device side is gm_nbr.h) and the pair-score launch (pair_scores.hip), for the translation units that read the one
// and score pairs of their own through the other (candidates.hip)
int gm_nbr_index(const gm_store* s);                                                      // builds the index at first use (under gm_store::nbr_mu); complete on the device on return
void gm_nbr_release(const gm_store* s);                                                   // frees the index's five device arrays (a failed build, gm_store_destroy)
int gm_pair_lanes(const gm_store* s, int32_t g, const char* what, int* lpp);              // GM_EINVAL for a pair_lanes knob that is no instantiation; *lpp (optional; needs the index) = the lanes per pair in force
int gm_pair_scores_launch(const gm_store* s, int32_t g, int lpp, const int32_t* d_pairs, int64_t n, int mask, float* d_out, hipStream_t st);      // k_pair_scores<lpp> over n pairs of graph g

// ---- the ranking of candidate partners, device side, for the two translation units that select them (candidates.hip: gm_store_pair_candidates;
// pagerank_candidates.hip: gm_store_pagerank_candidates): the key of include/gmeta_hip.h, the workgroup scan of the radix select, and the sort of the
// survivors with the padding behind them.  Workgroups of GM_CAND_THREADS threads.
#define GM_CAND_THREADS 256
#define GM_CAND_WAVES (GM_CAND_THREADS / GM_WAVE)
#define GM_CAND_MAX_K 1024

// (uint64(score bits) << 32) | (0xFFFFFFFF - w): descending key = descending score, equal scores by ascending node id
__device__ __forceinline__ unsigned long long gm_cand_key(uint32_t score_bits, int32_t w) {
    return ((unsigned long long)score_bits << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)w);
}

// inclusive prefix of v over the workgroup's threads; *total = the sum.  part: GM_CAND_WAVES ints of LDS; two barriers
__device__ __forceinline__ int gm_cand_scan(int v, int* part, int* total) {
    const int lane = (int)threadIdx.x & (GM_WAVE - 1), wave = (int)threadIdx.x / GM_WAVE;
    int inc = v;
#pragma unroll
    for (int o = 1; o < GM_WAVE; o <<= 1) { const int t = __shfl_up(inc, o, GM_WAVE); if (lane >= o) inc += t; }
    __syncthreads();                                                            // (the previous use of part is over)
    if (lane == GM_WAVE - 1) part[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < GM_CAND_WAVES; ++w) { const int p = part[w]; tot += p; if (w < wave) base += p; }
    *total = tot;
    return base + inc;
}

// sk[0 .. cnt) in LDS (sk: GM_CAND_MAX_K keys; cnt <= GM_CAND_MAX_K, complete behind a barrier of the caller's): the unique keys of a source's survivors in
// any order -> the result row at out_*[o .. o + k): the keys descending, -1 / 0.0f behind the last
__device__ __forceinline__ void gm_cand_sort_write(unsigned long long* sk, int cnt, int k, int64_t o, int32_t* __restrict__ out_nodes, float* __restrict__ out_scores) {
    const int tid = (int)threadIdx.x;
    int S = 1;
    while (S < cnt) S <<= 1;
    for (int i = cnt + tid; i < S; i += GM_CAND_THREADS) sk[i] = 0ull;          // below every key: a candidate's score bits are positive
    __syncthreads();
    for (int size = 2; size <= S; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (S >> 1); t += GM_CAND_THREADS) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i + stride;
                const unsigned long long x = sk[i], y = sk[j];
                const bool desc = (i & size) == 0;
                if (desc ? x < y : x > y) { sk[i] = y; sk[j] = x; }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += GM_CAND_THREADS) {
        const unsigned long long key = j < cnt ? sk[j] : 0ull;
        out_nodes[o + j] = j < cnt ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        out_scores[o + j] = j < cnt ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    }
}

// What every store-level link-prediction call checks first: the store, the graph and -- with cnt_name, the count's name in the call's signature -- the count
// 0 .. INT32_MAX and the flag bits.  (gm_store_has_edges and gm_store_negative_pairs have count bounds of their own and pass no name.)
static inline int gm_store_call_check(const char* what, const gm_store* s, int32_t g, const char* cnt_name = nullptr, int64_t n = 0, int32_t flags = 0) {
    GM_REQUIRE(s, GM_EINVAL, "%s: store is NULL", what);
    GM_REQUIRE(g >= 0 && g < s->n_graphs, GM_EINVAL, "%s: graph %d of a store with %d graph(s)", what, g, s->n_graphs);
    if (!cnt_name) return GM_OK;
    GM_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, GM_EINVAL, "%s: %s = %lld", what, cnt_name, (long long)n);
    GM_REQUIRE((flags & ~GM_PAIR_MASK_TARGET) == 0, GM_EINVAL, "%s: unknown flag bits 0x%x (GM_PAIR_MASK_TARGET = 1)", what, (unsigned)flags);
    return GM_OK;
}

// ---- host phase timing for the setup paths (env GM_TIMING=1 prints to stderr)
#include <chrono>
struct gm_phase_timer {
    const char* what; bool on; std::chrono::steady_clock::time_point t0, t;
    explicit gm_phase_timer(const char* w) : what(w) {
        on = gm_knob().timing != 0; t0 = t = std::chrono::steady_clock::now();
    }
    void lap(const char* phase) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[gm timing] %s/%s %.1f us\n", what, phase, std::chrono::duration<double, std::micro>(n - t).count());
        t = n;
    }
    ~gm_phase_timer() {
        if (on) fprintf(stderr, "[gm timing] %s total %.1f us\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// ---- device allocation helpers (stream-ordered pool so that per-batch builds do not sync the device)
int gm_dev_alloc(void** p, size_t bytes, hipStream_t s);
void gm_dev_free(void* p, hipStream_t s);
// big, batch-lived blocks: a process-level cache in front of the stream-ordered pool (common.hip: why); *cap >= need
int gm_slab_acquire(char** base, size_t* cap, size_t need, hipStream_t s);
void gm_slab_release(char* base, size_t cap, hipStream_t s);
template <class T>
static inline int gm_alloc(T** p, size_t n, hipStream_t s) { return gm_dev_alloc((void**)p, (n ? n : 1) * sizeof(T), s); }

// ---- pinned staging for batch builds.  A hipMemcpyAsync from / to PAGEABLE host memory waits for the stream on the host (and the callers used
// to add a hipStreamSynchronize so that their std::vectors could go out of scope): every small table of a batch build was a host round trip,
// and under a saturated GPU (extraction prefetched while a meta-step runs) each round trip waits for the build's kernel to get a CU -- ~20 of them
// made one extraction as long as the meta-step it was meant to hide behind.  A gm_stager hands out pinned host memory from a per-thread pool;
// copies through it are truly asynchronous and the memory returns to the pool once the stream has passed the stager's end.
struct gm_stager {
    hipStream_t s;
    std::vector<int> used;           // pool chunks this build holds
    char* cur = nullptr; size_t left = 0;
    explicit gm_stager(hipStream_t st) : s(st) {}
    ~gm_stager();
    gm_stager(const gm_stager&) = delete;
    gm_stager& operator=(const gm_stager&) = delete;
    void* take(size_t bytes);                                        // pinned, 64-byte aligned; NULL when the host allocation fails
    int upload(void* dptr, const void* src, size_t bytes);           // src (any host memory) -> staging -> device, asynchronous
    template <class T> int upload(T* dptr, const std::vector<T>& v) { return v.empty() ? GM_OK : upload((void*)dptr, (const void*)v.data(), v.size() * sizeof(T)); }
    template <class T> T* download(const T* dsrc, size_t n) {        // device -> pinned (valid after the caller synchronises `s`); NULL on failure
        T* h = (T*)take((n ? n : 1) * sizeof(T));
        if (h && n && hipMemcpyAsync(h, dsrc, n * sizeof(T), hipMemcpyDeviceToHost, s) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return h;
    }
};

// ---- device scratch of one call: taken from the stream-ordered pool and handed back to it on the call's stream, whichever way the call ends
struct gm_scratch {
    hipStream_t st;
    std::vector<void*> p;
    explicit gm_scratch(hipStream_t s) : st(s) {}
    ~gm_scratch() { for (void* q : p) gm_dev_free(q, st); }
    gm_scratch(const gm_scratch&) = delete;
    gm_scratch& operator=(const gm_scratch&) = delete;
    template <class T> int take(T** d, size_t n) {
        GM_TRY(gm_alloc(d, n, st));
        p.push_back((void*)*d);
        return GM_OK;
    }
    template <class T> int put(T** d, const std::vector<T>& v, gm_stager& sg) {
        GM_TRY(take(d, v.size()));
        return sg.upload(*d, v);
    }
};

// ---- the selection of gm_store_pagerank_candidates (pagerank_candidates.hip), run by the export in pair_pagerank.hip on every round of its walk
struct gm_nbr_graph;
struct gm_pprc {                         // one call's selection scratch, sized for its widest round
    int32_t k = 0, wgs_max = 0; hipStream_t st = nullptr;
    void* cols = nullptr;                // [Bmax] per-column state of the radix select
    int32_t *hist = nullptr, *cnt = nullptr, *total = nullptr, *ties = nullptr;      // [256, Bmax] bins; [Bmax] survivors; [Bmax] |R|; [ranges, Bmax] threshold entries per row range
    unsigned long long* surv = nullptr;  // [Bmax, GM_CAND_MAX_K] the survivors' keys
};
int gm_pprc_prepare(gm_pprc* w, gm_scratch& sc, int32_t Bmax, int32_t k, hipStream_t st);
// P[N, Br]: the round's state (overwritten: the exclusions), d_src[Br]: its columns' sources (-1: none); the `rows` output rows d_row[.] take the columns d_col[.] - c0
// (d_col < 0: a source outside the graph).  tm: the phase laps walk / exclusion / select, the stream synchronised behind each (NULL: none)
int gm_pprc_round(const gm_pprc& w, const gm_nbr_graph& G, float* P, int32_t Br, const int32_t* d_src, const int32_t* d_row, const int32_t* d_col, int64_t c0, int64_t rows,
                  int32_t* d_out_nodes, float* d_out_scores, int32_t* d_out_total, gm_phase_timer* tm);

// ---- the planes and the count of gm_store_pair_distance_profile (distance_profile.hip), run by the export in pair_distance.hip on every level of its search
// next[N, W]: a level's new bits, one word per (node, 64 columns); flag[0] == 0 on the device: the level found none -> plane[64 W, ceil(N / 64)]: one word per
// (column, 64 nodes), written where a bit is set (the caller zeroed it)
int gm_prof_transpose(hipStream_t st, const uint64_t* next, int32_t W, int64_t N, const int32_t* flag, uint64_t* plane);
// T[D + 1, B, ceil(N / 64)]: the planes of the levels 0 .. D of B columns; entry e = the pair of the columns cu[e], cv[e] -> out[dst[e], D + 2, D + 2]
int gm_prof_count(hipStream_t st, const uint64_t* T, int32_t D, int64_t B, int64_t N, const int32_t* cu, const int32_t* cv, const int64_t* dst, int64_t cnt, int32_t* out);

// ---- layout helpers
struct gm_layout {
    int n_gcn;
    int dims[GM_MAX_GCN + 1];
    int n_out, link, hc;              // hc = width of the head input
    int readout;                      // GM_READOUT_* of the calling thread when the layout was made (gm_set_readout): under MEAN hc = dims[n_gcn] whatever `link` says
    int64_t w_off[GM_MAX_GCN], b_off[GM_MAX_GCN], wl_off, bl_off, P;
};
int gm_make_layout(const gm_model_t* m, gm_layout* L);
// dims[0] of a model against the feature rows of a batch (the padded width is what the kernels' internal model carries)
static inline int gm_check_feat_dim(const gm_batch* b, int dims0, const char* what) {
    if (dims0 == b->feat_dim || dims0 == b->feat_ld) return GM_OK;
    if (b->hop_D) gm_set_error("%s: dims[0]=%d but the batch has %d features (%d of the store + %d hop-label columns, gm_set_hop_labels(%d))", what, dims0, b->feat_dim,
                               b->store->feat_dim, b->feat_dim - b->store->feat_dim, b->hop_D);
    else gm_set_error("%s: dims[0]=%d but the store has %d features", what, dims0, b->feat_dim);
    return GM_EINVAL;
}
static inline int gm_pad_feat(int F) { return F <= 32 ? 32 : (F + 63) / 64 * 64; }

// ---- kernels launched across translation units
// Generic CSR aggregate: out[r,:] = epi( s_out[r] * sum_{c in row r} s_in[c] * x[src(c),:] ).
struct gm_agg_args {
    const int32_t* indptr;
    const int32_t* indices;
    const float* x;            // [*, ldx]
    const int32_t* x_row;      // optional indirection applied to the column index (feature gather)
    const float* e_w;          // optional per-edge source scale (= s_in[indices[e]]; gm_batch::d_enorm): replaces the s_in gather
    const int32_t* x_idx;      // optional per-edge source row of x (= x_row[indices[e]]; gm_batch::d_efeat): replaces the x_row gather
    int skip_on, skip_lo, skip_hi;   // window kernel only, with skip_on: leave rows with skip_lo <= degree <= skip_hi unwritten (the fused aggregate + GEMM forms them)
    int64_t ldx;
    const float* s_in;         // optional per-source scale
    const float* s_out;        // optional per-destination scale
    int keep_signed;           // s_out carries "nobody reads this row of `out`" in its sign bit (gm_batch::d_norm_e1): the scale is the magnitude, a flagged row is not stored -- computed only where the launch writes relu_bits, left at its descriptor otherwise
    const float* mask_h;       // optional [rows, width]: zero the output where mask_h <= 0 (relu')
    const uint8_t* mask_b;     // same mask, packed: byte (row*width + col)/4 holds the relu' bits of 4 consecutive columns
    uint8_t* relu_bits;        // optional output: packed relu' bits of `out` (written with relu; width % 4 == 0)
    const float* bias;         // optional per-set bias (bias + set*bias_stride) -- matmul-first layers
    int64_t bias_stride;
    const int32_t* set_row_off;// required when bias != NULL and bias_stride != 0: row range of every set
    int n_sets;
    int relu;
    float* out;                // [rows, width]
    int64_t rows;
    int width;
    const int32_t* heavy;      // optional list of rows with more than heavy_deg edges (processed by a whole workgroup)
    int n_heavy;
    int heavy_deg;
    const int32_t* sched;      // optional block schedule (gm_agg_schedule): hub rows ride in the window launch
    int sched_len, sched_win;
    const int32_t* hub; float* hub_scratch; int hub_part;     // with sched: hub rows split over several blocks (gm_agg_sched)
    const int32_t* rowlist; int64_t n_list; int list_win;      // window kernel only: the wave windows walk rowlist[0 .. n_list) instead of every row (sched / sched_len then index list blocks)
    const int32_t* n_list_dev; // optional, with rowlist: the list's true length on the device (<= n_list, which then is the host's bound: it sizes grid and schedule; the windows past the length leave at once)
    // optional: the batch / orientation whose stream tables this launch may use (gm_agg_stream_args): eligible launches take the LDS-DMA stream kernel (agg_stream.hip)
    const gm_batch* stream; int stream_o; int stream_feat; int64_t stream_xrows;
    int* launched;             // optional: receives the GM_AGG_ID_* of the instantiation launched (host side; tests)
};
// gm_agg_args::launched
#define GM_AGG_ID_LPR(LPR) ((LPR) == 64 ? 6 : (LPR) == 32 ? 5 : (LPR) == 16 ? 4 : (LPR) == 8 ? 3 : (LPR) == 4 ? 2 : 1)
#define GM_AGG_ID_ONE(VEC, LPR) (100 + ((VEC) == 4 ? 10 : 0) + GM_AGG_ID_LPR(LPR))      // k_agg<VEC, LPR>: 101 .. 106, 111 .. 116
#define GM_AGG_ID_WIN(LPR, NCH) (200 + 16 * ((NCH) == 2 ? 3 : GM_AGG_ID_LPR(LPR) - 4))  // k_agg_win<LPR, NCH>: 200, 216, 232, 248, plus the flags below
#define GM_AGG_ID_WIN_SCHED 1           // hub rows ride in the window launch (block schedule)
#define GM_AGG_ID_WIN_SPLIT 2           // ... split into parts (arrival ticket, part-order sum)
#define GM_AGG_ID_WIN_HEAVY 4           // hub rows by a separate k_agg_heavy<LPR, NCH> launch
#define GM_AGG_ID_WIN_LIST 8            // the windows walk a row list
#define GM_AGG_ID_STREAM(LPR, SPLIT) (300 + 2 * (GM_AGG_ID_LPR(LPR) - 4) + ((SPLIT) ? 1 : 0))      // k_agg_stream<LPR, .>: 300 .. 305
// fills the stream fields of `a` for orientation o of batch b (gather: the sources are rows of the store's feature table); a no-op without tables
int gm_agg_stream_args(gm_agg_args& a, const gm_batch* b, int o, bool gather, hipStream_t s);      // (builds the orientation's tables at first use, on s)
bool gm_stream_ok(const gm_agg_args& g);
bool gm_stream_batch_ok(const gm_batch* b, int o);      // the batch is of the kind that gets stream tables (built at first use)
int gm_launch_stream(const gm_agg_args& g, int nt, hipStream_t s);
int gm_stream_tables(gm_batch* b, int o, const int32_t* hubs_host, const int32_t* deg_host, int n_hubs, int n_parts, const std::vector<int32_t>* part_tab, hipStream_t s,
                     gm_stager* sg);
#define GM_FUSE_SELF 0x40000000   // gm_batch::d_fuse2 entry: the source is the row's own, already aggregated, row
#define GM_FUSE_ZERO 0x20000000   // ... the row has no source: an all-zero row
const float* gm_zero_row(hipStream_t s);   // 4096 zero floats on the current device (allocated once)
#ifndef GM_ZERO_ROWS
#define GM_ZERO_ROWS 1            // rows of the zero block behind the dense backward's T (a power of two; gm_batch::d_ect spreads the dead sources over them)
#endif
#define GM_FUSE_MAXDEG 2
#define GM_AGG_HUB_LD 512      // floats per partial hub row (the widest window-kernel width)
struct gm_agg_sched { int32_t* d_sched = nullptr; int32_t len = 0; int32_t* d_hub = nullptr; float* d_hub_scratch = nullptr; int32_t hub_part = 0; int32_t hub_words = 0, parts = 0;
                      std::vector<int32_t> tab; };      // tab: the host copy of the part table (gm_agg_schedule_flat builds further schedules over the same parts)
int gm_batch_hub_order(const gm_batch* b, int o, hipStream_t s, int set = 0);
int gm_batch_hub_alt(const gm_batch* b, hipStream_t s);      // allocates the second counter / partial-row set (once)
template <class A> inline int gm_agg_hub(A& a, const gm_batch* b, int o, hipStream_t s, int set = 0) {
    const bool alt = set == 1 && b->d_hub2[o];
    a.hub = alt ? b->d_hub2[o] : b->d_hub[o]; a.hub_scratch = alt ? b->d_hub_scratch2[o] : b->d_hub_scratch[o]; a.hub_part = b->hub_part[o];
    return a.hub ? gm_batch_hub_order(b, o, s, alt ? 1 : 0) : GM_OK;
}
// Rows per wave window for a launch over `rows` rows (64 at most, halved until the launch has enough waves).
int gm_agg_window(int64_t rows, int64_t edges);
// Block schedule for the window aggregate over `rows` rows with the given (ascending, host) hub-row list: 8 per-XCD lists of
// equal length out->len; entry >= 0: window block id, <= -2: hub part -(entry) - 2 (hub row heavy[..] itself when the rows are not
// split: out->d_hub == NULL), -1: nothing.  A hub row's blocks follow the window block that contains the row, on the XCD whose L2 is
// streaming that subgraph.  heavy_deg_host: the rows' edge counts (NULL: never split).
struct gm_stager;
// Only the flat block schedule, for hub rows at (virtual, ascending) positions pos[] among `rows` window rows, over the part table `tab` of an earlier
// gm_agg_schedule call (empty: one block per hub row)
// keep (or NULL: all): one byte per hub row, 0 = the row gets no block in this schedule (a launch in which the host knows it to have no work)
int gm_agg_schedule_flat(gm_batch* b, int64_t rows, int win, const int32_t* pos, int n_heavy, const std::vector<int32_t>& tab, int32_t** d_sched, int32_t* len, hipStream_t s, gm_stager* sg,
                         const uint8_t* keep = nullptr);
int gm_agg_schedule(gm_batch* b, int64_t rows, int win, const int32_t* heavy_host, const int32_t* heavy_deg_host, int n_heavy, gm_agg_sched* out, hipStream_t s, gm_stager* sg);
int gm_heavy_deg();   // rows with more edges than this are aggregated by a whole workgroup (64; a batch's own threshold is by density, see gm_heavy_deg_for)
int gm_heavy_deg_for(int64_t rows, int64_t edges);
int gm_launch_aggregate(const gm_agg_args& a, hipStream_t s);

// Grouped GEMM  C[rows of set t] = epi( A[rows] @ op(B_t) ),  A [rows,K] (lda), C [rows,N] (ldc).
struct gm_gemm_args {
    const float* A; int64_t lda;
    const float* B; int64_t b_stride;   // B_t = B + t*b_stride ; [K,N] row-major, or [N,K] when transB
    int transB;
    float* C; int64_t ldc;
    int K, N;
    const float* row_scale;             // optional: C *= row_scale[row] (before bias)
    const float* row_scale_keep;        // optional, split kernels only (others ignore it): |value| = row_scale, sign bit set = nobody reads this row of C: it is computed and
                                        //   not stored (the h[to_fetch] select of Classifier.forward, learner.py, fused into the last layer's epilogue); n_keep = rows stored (accounting)
    int64_t n_keep;
    const float* bias; int64_t bias_stride;   // optional per-set bias [N]
    int relu;
    const float* mask_h;                // optional [rows, ldc]: zero C where mask_h <= 0 (relu')
    const uint8_t* mask_b;              // same mask packed, byte (row*ldc + col)/4 = bits of 4 consecutive columns (needs vector stores)
    uint8_t* relu_bits;                 // optional output: packed relu' bits of C (with relu; N % 4 == 0, ldc == N)
    const uint16_t* Bsplit; int64_t bsplit_stride;   // optional: B_t as three bf16 planes (gm_split_weights) -> the split-bf16 kernel (gemm_split.h)
    // with Bsplit: fused aggregate + GEMM.  fuse2 = gm_batch::d_fuse2 / d_fuse2_feat; A / lda then address the aggregate's INPUT rows
    // (previous layer's output or the feature table) and rows the table flags GM_FUSE_SELF read their finished aggregate from zside
    const void* fuse2; const float* zside; int64_t ldz;
    // split kernel with two fp16 pieces per operand (np = 2; 0 / 3 = three bf16 pieces): Bsplit then holds fp16 planes made under b_bound, and
    // a_bound bounds the A rows (gm_bound.h).  amax_out (np = 2 only): per-set slots that receive the largest |C| stored (atomicMax on zeroed slots)
    int np; gm_bound a_bound, b_bound; unsigned* amax_out;
    float* zero_out;                    // also zero-fill this [rows, ldc] buffer (dQ of the backward pass that follows): in the epilogue of the split / DMA kernels, a memset on the other paths
    const int32_t* tiles;               // device [n_tiles*3]: set, row0, nrows  (nrows <= BM)
    int n_tiles;
    int64_t rows;                       // total rows covered by the tiles (profiling: flops = 2*rows*K*N)
    const int32_t* tile_live;           // optional, with row_scale_keep: one word per tile, 0 = the tile holds no kept row (gm_batch::d_tile_live).  Taken by the fused three-piece split kernels
                                        //   where the launch writes neither relu_bits nor zero_out (gemm_split.h: SplitGemmK::tile_live); every other launch ignores it
    const gm_batch::pack_set* pack;     // optional, in tile_live's place (same conditions): the row set's packed tiles (gm_batch::pack).  Taken where row_scale_keep is the set's keep vector and
                                        //   fuse2 one of the tables it carries in packed order; every other launch ignores it
    int grid_test;                      // tests only (gm_dense_fused_gemm_rows): workgroups of a fused split launch; 0 = the production rule
    int* launched;                      // optional: receives the GM_GEMM_ID_* of the instantiation launched (host side).  Set only by the
                                        // numerics-test export gm_dense_gemm; the product path leaves it NULL
};
// gm_gemm_args::launched
#define GM_GEMM_ID_GLDS4 1              // k_gemm_glds<2, 4, 2>
#define GM_GEMM_ID_GLDS2 2              // k_gemm_glds<2, 2, 2>
#define GM_GEMM_ID_GLDS1 3              // k_gemm_glds<2, 1, 2>
#define GM_GEMM_ID_GLDS_SMALL 4         // k_gemm_glds<4, 2, 1>
#define GM_GEMM_ID_NN(WC, VEC, TB) (10 + 4 * ((WC) == 4 ? 2 : (WC) == 2 ? 1 : 0) + 2 * (VEC) + (TB))     // k_gemm_nn<WC, VEC, TB>: 10 .. 21
#define GM_GEMM_ID_SPLIT(GATHER, MI, WC, NP) (30 + 10 * (GATHER) + ((MI) == 2 ? 0 : (WC) == 4 ? 2 : 4) + ((NP) == 2))   // k_gemm_split_p: 30 .. 35, 40 .. 45
#define GM_GEMM_BM 128
int gm_launch_gemm_nn(const gm_gemm_args& a, hipStream_t s);
// fp32 GEMM on the bf16 matrix cores by exact 3-way operand splitting (gemm_split.h): eligibility of a launch and the weight planes.
// gm_gemm_mode(): 0 = exact-fp32 MFMA kernels only, 1 = split-bf16 kernel where eligible (env GM_GEMM_MODE=f32|split, gm_set_gemm_mode).
int gm_gemm_mode();
bool gm_gemm_split_ok(int n_tiles, int K, int N);
// np = 3: three bf16 planes; np = 2: two fp16 planes under `bound` (per-set stride 3 planes either way)
int gm_split_weights(const float* params, int64_t pstride, int64_t w_off, int K, int N, int trans, int sets, uint16_t* out, hipStream_t s, int np = 3,
                     gm_bound bound = gm_no_bound());
// out[t * out_stride] = max(out[...], max_i |x[t * stride + off + i]|), i < n, as fp32 bit patterns (the slots must have been zeroed)
int gm_amax(const float* x, int64_t stride, int64_t off, int64_t n, int sets, unsigned* out, int64_t out_stride, hipStream_t s);
int gm_amax_segs(const float* x, const int64_t* off, const int64_t* n, int segs, unsigned* out, int64_t out_stride, hipStream_t s);   // up to 8 segments of x, one launch
int gm_split_np();                      // pieces per operand of the split kernels: 3 (bf16 triple, default) or 2 (opt-in fp16 pair, only where bounds are recorded); env GM_SPLIT_PIECES

// Grouped transposed-A GEMM for weight gradients:
//   dW_t[K,N] = sum_{rows of set t} a_scale[row] * A[row,:]^T  G[row,:]   and   db_t[N] = sum G[row,:]
// computed as per-chunk partials followed by a deterministic reduction that also applies `beta`:
//   out_t = (beta_is_sgd ? w_t - lr * sum : sum)
// Reductions held back by gm_launch_wgrad (hold_this) until a later call on the same batch flushes them together with its own
// (k_wgrad_reduce_n): opaque argument blocks, filled and consumed by gemm.hip.
struct gm_wgrad_hold { int n = 0; int sets[GM_MAX_GCN] = {}; alignas(16) unsigned char slot[GM_MAX_GCN][256] = {}; };
struct gm_wgrad_args {
    const float* A; int64_t lda; int K;
    const int32_t* a_row;               // optional row indirection for A (layer-1 feature gather)
    const float* G; int64_t ldg; int N;
    const float* Gb; int64_t ldgb;      // optional: matrix whose column sums give db (default: G)
    const float* a_scale;               // optional
    const int32_t* chunks;              // device [n_chunks*3]: set, row0, nrows
    int n_chunks;
    const int32_t* set_chunk_off;       // device [sets+1]: chunk range per set
    int sets;
    float* partial;                     // workspace [n_chunks, (K+1)*N]  (row K = bias partial)
    float* dW; int64_t dw_stride;       // dW_t = dW + t*dw_stride   [K,N]
    float* db; int64_t db_stride;       // db_t                      [N]
    // optional fused inner-loop SGD (meta.py:126,151): next_t[off + j] = cur_t[off + j] - lr * grad, written together with the gradient
    const float* sgd_cur; int64_t sgd_cur_stride; float* sgd_next; int64_t sgd_next_stride; float sgd_lr;
    int64_t w_off, b_off;               // offsets of this layer's W and b inside a parameter vector
    // two fp16 pieces per operand (np = 2) in the split weight-gradient kernel: bounds of A and G.  With planes: pl_np = 2 writes fp16 planes
    // under pl_bound
    int np; gm_bound a_bound, g_bound; int pl_np; gm_bound pl_bound;
    uint16_t* pl_fwd; uint16_t* pl_dz;  // optional (with sgd_next): the updated W also written as split-bf16 planes for the NEXT step's GEMMs
                                        // ([set][3][K/8][N][8] for X @ W, [set][3][N/8][K][8] for dQ @ W^T; gemm_split.h layouts): no k_split_w launches
    float* wt_next;                     // optional (with sgd_next): the updated W also written transposed, [set][N][K] -- what the NEXT
                                        // step's dZ GEMM (dQ @ W^T on the row-major DMA kernel) reads, instead of a transpose launch
    int64_t rows;                       // total rows covered by the chunks (profiling: flops = 2*rows*K*N)
    // optional (split kernel only: gm_wgrad_gather_ok): A = Z of a pass whose forward ran the FUSED aggregate + GEMM -- rows of one or two sources are formed
    // from gx (row stride ldgx) through the per-row table fuse2 (gm_batch::d_fuse2 / d_fuse2_feat) in the aggregate's fma order, rows the table flags
    // GM_FUSE_SELF are read from A (the partial aggregate launch wrote them), GM_FUSE_ZERO rows are zero
    const void* fuse2; const float* gx; int64_t ldgx;
    int64_t a_rows;                     // launch accounting only (GM_PROF_WGRAD_BYTES): rows of A the launch fetches, where the table sends the others to the zero row (0 = every row)
    // optional (three-piece split kernel only, GM_EINVAL elsewhere): the row scale again, |value| = a_scale, with the SIGN BIT SET on rows of G that were never
    // written (dQ_L outside the centre rows: gm_batch::d_norm_c) -- such a row enters dW and db as zeros, whatever its bytes hold
    const float* g_keep;
    gm_wgrad_hold* hold; int hold_this; // optional: hold this call's reduction back (hold_this = 1; its `partial` must then stay untouched) /
                                        // flush the held ones with this call's reduction (hold_this = 0)
    int pick;                           // kernel family: 0 = the library's choice (gm_gemm_mode, GM_WGRAD_SPLIT_MIN_CHUNKS); GM_WGRAD_PICK_EXACT /
                                        // GM_WGRAD_PICK_SPLIT force one (GM_EINVAL where the split kernel cannot take the call).  Set only by the
                                        // numerics-test export gm_dense_wgrad; the product path leaves it 0
};
#define GM_WGRAD_PICK_EXACT 1           // k_wgrad_fast / k_wgrad, whatever the launch size and gm_gemm_mode()
#define GM_WGRAD_PICK_SPLIT 2           // k_wgrad_split, whatever the launch size and gm_gemm_mode()
#define GM_WGRAD_ROWS 1024
int gm_launch_wgrad(const gm_wgrad_args& a, hipStream_t s);
bool gm_wgrad_gather_ok(int n_chunks, int K, int N);

// ---- The launches of the model's schedules, named once.  Defined in model.hip; the dense schedule (gcn_forward / gcn_backward and their step functions), the cone
// schedule, the row-sparse backward and the gm_dense_* exports (dense_exports.hip: what the fp64 numerics and the dead-row suites drive) all fill these field groups
// through these builders and nowhere else, so a field a production launch gains is a field of the launch the tests check
// A row set of a batch, as its tables carry it (row_view): every row; the rows with an out-edge inside the batch (the only rows of H_l below the last layer that an
// edge reads); the sources of the centres' in-edges; the centre rows
enum RowSet { ROWS_ALL, ROWS_SRC, ROWS_E1, ROWS_CENTRE };
// A row set as the launches take it.  keep: the row scale with "not of the set" in its sign bit -- gm_gemm_args::row_scale_keep (rows a GEMM stores), gm_wgrad_args::g_keep
// (rows of G that were written), gm_agg_args::s_out + keep_signed of a transposed aggregate (NULL: every row).  sign: +1 on the set, -1 off it -- s_out + keep_signed of a
// forward partial aggregate, a scale of exactly 1 (NULL: every row).  tab: the per-row source table of a fused loader or a table-fed weight gradient over a Z_l formed on the
// set -- the full table's entry on its rows, the zero row everywhere else (gather: the layer reads the feature table; a centre-restricted layer never does, plan_check).
// obs: the set's index into the tables of gm_batch_fwd_counts, -1 where it has none.  n: its rows as the host knows them (ROWS_E1: a bound, see rows_kept in model.hip)
// live: one word per GEMM row tile, 0 = no row of the set in it (gm_batch::d_tile_live; NULL: every row / no flags)
// pack: the set's packed tiles (gm_batch::pack; NULL: every row / the batch carries none)
struct RowView { const float* keep; const float* sign; const void* tab; int obs; int64_t n; const int32_t* live; const gm_batch::pack_set* pack; };
RowView row_view(const gm_batch* b, RowSet rs, bool gather);
// The rows a GEMM or a weight gradient runs over: their norm, GEMM row tiles, weight-gradient chunks and count.  The batch is one such level (batch_level); the cone
// schedule has one per layer boundary and the row-sparse backward two compact ones (model.hip)
struct LevelView { const float* norm; const int32_t* tiles; int n_tiles; const int32_t* chunks; const int32_t* set_chunk_off; int n_chunks; int64_t rows; int sets; };
LevelView batch_level(const gm_batch* b);
void gemm_rows(gm_gemm_args& g, const LevelView& v);       // row_scale, tiles, n_tiles, rows
void wgrad_rows(gm_wgrad_args& w, const LevelView& v);     // a_scale, chunks, n_chunks, set_chunk_off, sets, rows
// a GEMM that stores the rows of a set only (keep: row_scale_keep + the kept-row count of the launch accounting) and / or takes the set's tile flags (live) and, with
// them, the set's packed tiles (pack: GM_PACK_ROWS)
void gemm_keep_rows(gm_gemm_args& g, const RowView& v, bool keep, bool live, int64_t n_keep, bool pack = false);
// the dZ GEMM over a dQ_L that holds its centre rows only: the fused loader reads them through gm_batch::d_dq_tab and zeros for every other row
void gemm_dq_table(gm_gemm_args& g, const gm_batch* b, const float* dQ, int64_t ld);
// orientation dir of the batch (0: A, the in-edges; 1: A^T) as an aggregate walks it -- CSR, rows, hub-row list, the edges' weights of a weighted batch (agg_graph) -- and
// with the orientation's block schedule and hub set hub_set on top: the batch-wide aggregate of the dense schedule (batch_agg)
void agg_graph(const gm_batch* b, int dir, gm_agg_args& a);
int batch_agg(const gm_batch* b, int dir, int hub_set, hipStream_t st, gm_agg_args& a);
// a restricted launch over one of the batch's lists of observable rows: the list in the windows' place, its own schedule (or none), the length the device counted
void agg_take_list(gm_agg_args& a, const gm_batch::obs_list& ol);
// the last layer's transposed aggregate over a T_L that holds its centre rows only: T_L read through gm_batch::d_ect; out != ROWS_ALL: only that set's rows of dQ_{L-1}
// stored (s_out = the set's keep vector, keep_signed)
void agg_centre_t(gm_agg_args& a, const gm_batch* b, RowSet out);
int gm_gather_rows(const gm_batch* b, const int32_t* feat_row, int64_t n, int F, float* out, hipStream_t st);      // extract.hip: out[i, :F] = feature row feat_row[i] of the store

// Rows per weight-gradient chunk for sets of the given sizes.  One workgroup (one CU: 128 accumulator VGPRs x 16 waves)
// takes one chunk and writes a (K+1)xN partial, so the chunk count should sit just under a multiple of the CU count (256) --
// 280 chunks cost two rounds for the work of 1.1 -- and be small: every chunk adds a partial to write and re-read.
// Chunks never straddle two sets (per-task weights).  Returns a multiple of 32.
int gm_num_cus();                         // compute units of the current device (cached per device)
int gm_func_full_lds(const void* fn);     // allow 160 KiB of dynamic LDS for a kernel, once per (device, kernel)
#define GM_WGRAD_EXTRA_ROUND_PCT 25   // percent of row-slot efficiency another round of chunks must gain over fewer, longer chunks
static inline int gm_wgrad_chunk_rows(const std::vector<int32_t>& set_off, int n_cu = gm_num_cus()) {
    const int sets = (int)set_off.size() - 1;
    int64_t total = 0; int mx = 1;
    for (int t = 0; t < sets; ++t) { const int n = set_off[t + 1] - set_off[t]; total += n; mx = n > mx ? n : mx; }
    if (total <= 0) return 128;
    auto chunks_at = [&](int cr) { int64_t c = 0; for (int t = 0; t < sets; ++t) c += (set_off[t + 1] - set_off[t] + cr - 1) / cr; return c; };
    int best = 128; double best_eff = -1.0;
    for (int rounds : {1, 2, 3, 4, 6, 8}) {
        const int64_t cap = (int64_t)n_cu * rounds;
        int lo = 1, hi = (mx + 31) / 32;                 // in units of 32 rows; chunks_at(32*hi) == #non-empty sets
        if (chunks_at(32 * hi) > cap) continue;          // more sets than workgroup slots at this round count
        while (lo < hi) { const int mid = (lo + hi) / 2; if (chunks_at(32 * mid) <= cap) hi = mid; else lo = mid + 1; }
        const int cr = std::max(128, 32 * lo);
        const int64_t c = chunks_at(cr);
        const double eff = (double)total / ((double)((c + n_cu - 1) / n_cu) * n_cu * cr);   // useful rows / rows the rounds have room for
        if (eff > best_eff + 0.01 * GM_WGRAD_EXTRA_ROUND_PCT) { best_eff = eff; best = cr; }
    }
    return best;
}

// launch profiling by category (bench.py): work = algorithmic bytes (aggregate) or flops (GEMM, weight gradient)
#define GM_PROF_AGG 0
#define GM_PROF_GEMM 1
#define GM_PROF_WGRAD 2
#define GM_PROF_AGG_STRICT 3   // work-only shadow of GM_PROF_AGG: compulsory HBM bytes (a layer-1 gather reads at most the feature table)
#define GM_PROF_GEMM_SPLIT 4   // grouped GEMM launches that ran on the split-bf16 kernel (6 bf16 MFMA flops per fp32 flop; work = fp32 flops)
#define GM_PROF_WGRAD_SPLIT 5  // weight gradients on the split-bf16 kernel
#define GM_PROF_GEMM_SPLIT16 6 // grouped GEMMs on the two-piece fp16 split kernel (3 fp16 MFMA flops per fp32 flop)
#define GM_PROF_WGRAD_SPLIT16 7
#define GM_PROF_STEP_CATS 8     // categories of gm_meta_step (reset at the start of every step)
#define GM_PROF_EX_NODES 8      // extraction, phase A: k_nodes (BFS, sampling, node lists, induced degrees); work = subgraphs
#define GM_PROF_EX_FILL 9       // extraction, phase B: k_fill (batched CSR in both orientations, parents, norms, centres); work = subgraphs
#define GM_PROF_EX_FINAL 10     // batch finalisation (launch tables, hub schedule, gains, per-edge / per-row tables): GPU span incl. the host round trips inside it
#define GM_PROF_GEMM_SPLIT_BYTES 11   // work-only shadow of the split GEMM launches (categories 4 and 6): compulsory HBM bytes 4 rows (K + N) -- the A operand read once, C written once
#define GM_PROF_AGG_BOUND 12          // work-only shadow of category 0 with the partial launches priced as in rounds 2-3 (sources = min(edges, rows), an upper bound)
#define GM_PROF_GEMM_BYTES 13         // work-only shadow of EVERY grouped GEMM launch (categories 1, 4, 6): compulsory HBM bytes, A rows read once + the C rows it stores
#define GM_PROF_WGRAD_BYTES 14        // ... of every weight-gradient launch (categories 2, 5, 7): the A and G rows read once
#define GM_PROF_HEAD 15               // head + prototypical loss (+ head backward) launches: time; work = subgraphs
#define GM_PROF_READOUT 16            // mean readout, forward (k_readout_mean + k_readout_mean_fin): work = algorithmic bytes 4 rows Hd + 4 subs Hd
#define GM_PROF_READOUT_BWD 17        // mean readout, backward (k_readout_mean_bwd): work = algorithmic bytes 8 rows Hd + 4 subs Hd
#define GM_PROF_CATS 18
void gm_prof_begin(int cat, hipStream_t s, int64_t work);
void gm_prof_end(int cat, hipStream_t s);
void gm_prof_reset(int n_cats = GM_PROF_CATS);
void gm_prof_reset_cat(int cat);
bool gm_prof_enabled();
// distinct source rows of the in-edges of the rows with more than GM_FUSE_MAXDEG sources (what a partial aggregate launch reads): counted on the
// device at first use (a bitmap over the batch rows; synchronises the stream) -- only the launch accounting of bench.py asks for it
int64_t gm_batch_unfused_sources(const gm_batch* b, hipStream_t s);
// distinct source rows of the centres' in-edges (the rows gm_batch::d_norm_e1 keeps): read back at first use (synchronises the stream) -- the launch accounting and the tests ask for it
int64_t gm_batch_e1_rows(const gm_batch* b, hipStream_t s);
// what a forward-only partial aggregate launch touches at GM_DEAD_ROWS=3 (which: 0 the last layer, 1 the layer below): out[3] = {rows it writes (more than GM_FUSE_MAXDEG sources
// and gm_batch::d_obs[which] positive), their in-edges, their distinct sources}.  Counted at first use (synchronises the stream): the launch accounting and the tests ask for it
int gm_batch_fwd_counts(const gm_batch* b, int which, hipStream_t s, int64_t* out);
// by-source edges of those rows: counted on the device at first use (synchronises the stream) -- only the launch accounting asks for it; gm_batch::edges where it cannot be had
int64_t gm_batch_e1_edges(const gm_batch* b, hipStream_t s);
void gm_prof_note(int cat, int64_t work);      // adds work to a category without timing events
static inline void gm_prof_agg_begin(hipStream_t s, int64_t bytes) { gm_prof_begin(GM_PROF_AGG, s, bytes); }
static inline void gm_prof_agg_end(hipStream_t s) { gm_prof_end(GM_PROF_AGG, s); }
