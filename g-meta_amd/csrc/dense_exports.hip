// Single launches of the update GEMM, the dZ product, the weight gradient and the aggregates as the step functions of gcn_forward / gcn_backward (model.hip) issue them: the
// field groups those launches share come from model.hip's own builders (gm_internal.h), not from a restatement here.  Host code only.
#include <algorithm>
#include "gm_internal.h"

// Two-piece bounds (gm_bound.h) of a row-major operand, one per set: max |x| over each set's rows (with the padding between them) -> slots[t * GM_BOUND_PAD]
static int set_row_amax(const gm_batch* b, const float* x, int64_t ldx, int cols, unsigned* slots, hipStream_t st) {
    int rc = GM_OK;
    for (int t0 = 0; rc == GM_OK && t0 < b->sets; t0 += 8) {
        const int segs = std::min(8, b->sets - t0);
        int64_t xo[8], xn[8];
        for (int i = 0; i < segs; ++i) {
            const int64_t r0 = b->h_set_row_off[t0 + i], nr = b->h_set_row_off[t0 + i + 1] - r0;
            xo[i] = r0 * ldx; xn[i] = nr > 0 ? (nr - 1) * ldx + cols : 0;
        }
        rc = gm_amax_segs(x, xo, xn, segs, slots + (int64_t)t0 * GM_BOUND_PAD, GM_BOUND_PAD, st);
    }
    return rc;
}

// The scaffolding of the GEMM exports.  split: W (trans: stored [N, K] -- the planes are its own rows, as the dZ product's) as planes for the split kernels; np == 2: two
// fp16 pieces per operand under bounds taken here -- of A over ax (per_set: one per set, over each set's rows as gm_dense_wgrad does, slots [0, sets); else one for all
// of it, slot 0), then one per weight matrix.  The launch, the frees
static int launch_gemm(const gm_batch* b, gm_gemm_args& g, bool split, const float* W, int64_t w_stride, int trans, int np, const float* ax, int64_t ldax, bool per_set,
                       const char* who, hipStream_t st) {
    uint16_t* planes = nullptr; unsigned* slots = nullptr;
    int rc = GM_OK;
    if (split) {
        const int K = g.K, N = g.N, wsets = w_stride ? b->sets : 1, na = per_set ? b->sets : 1;
        rc = gm_alloc(&planes, (size_t)wsets * 3 * K * N, st);
        gm_bound wb = gm_no_bound();
        if (rc == GM_OK && np == 2) {
            rc = gm_alloc(&slots, (size_t)(na + wsets) * GM_BOUND_PAD, st);
            if (rc == GM_OK && hipMemsetAsync(slots, 0, sizeof(unsigned) * (na + wsets) * GM_BOUND_PAD, st) != hipSuccess) { gm_set_error("%s: memset failed", who); rc = GM_EHIP; }
            if (rc == GM_OK) rc = per_set ? set_row_amax(b, ax, ldax, K, slots, st) : gm_amax(ax, 0, 0, (int64_t)b->rows * K, 1, slots, 0, st);
            if (rc == GM_OK) rc = gm_amax(W, w_stride, 0, (int64_t)K * N, wsets, slots + (int64_t)na * GM_BOUND_PAD, GM_BOUND_PAD, st);
            wb.amax = slots + (int64_t)na * GM_BOUND_PAD; wb.stride = w_stride ? GM_BOUND_PAD : 0;
            g.np = 2; g.a_bound = gm_no_bound(); g.a_bound.amax = slots; g.a_bound.stride = per_set ? GM_BOUND_PAD : 0; g.b_bound = wb;
        }
        if (rc == GM_OK) rc = gm_split_weights(W, w_stride, 0, K, N, trans, wsets, planes, st, np, wb);
        g.Bsplit = planes; g.bsplit_stride = w_stride ? (int64_t)3 * K * N : 0;
    }
    if (rc == GM_OK) rc = gm_launch_gemm_nn(g, st);
    if (planes) gm_dev_free(planes, st);
    if (slots) gm_dev_free(slots, st);
    gm_batch_mark_use(b, st);
    return rc;
}
// the batch's rows under the export's own row scale
static LevelView scaled_level(const gm_batch* b, const float* s) { LevelView v = batch_level(b); v.norm = s; return v; }

// ================================================================================ dense update, exported for numerics tests
extern "C" int gm_dense_update(const gm_batch_t* b, const float* x, int32_t K, const float* W, int64_t w_stride, int32_t N, float* out, int32_t mode,
                               void* stream) {
    GM_REQUIRE(b && x && W && out && K >= 1 && N >= 1, GM_EINVAL, "dense_update: bad arguments");
    gm_gemm_args g{};
    g.A = x; g.lda = K; g.B = W; g.b_stride = w_stride; g.C = out; g.ldc = N; g.K = K; g.N = N;
    gemm_rows(g, scaled_level(b, nullptr));
    const bool split = mode == 1 || mode == 2 || (mode < 0 && gm_gemm_split_ok(b->n_tiles, K, N));
    if (split) GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 32, GM_EINVAL, "dense_update: the split kernels need N = 128 or 256 and K a multiple of 16 (>= 32)");
    // mode 2: one bound for all of x, one per weight matrix
    return launch_gemm(b, g, split, W, w_stride, 0, mode == 2 ? 2 : 3, x, K, false, "dense_update", (hipStream_t)stream);
}

// The same product with every field of gm_gemm_args that the forward and dZ GEMMs set: the epilogue options, a transposed W, strides, the
// choice of kernel family, and the instantiation that ran
extern "C" int gm_dense_gemm(const gm_batch_t* b, const float* x, int64_t ldx, int32_t K, const float* W, int64_t w_stride, int32_t trans_w, int32_t N,
                             float* out, int64_t ldc, const float* s, const float* s_keep, const float* bias, int64_t bias_stride, int32_t relu,
                             uint8_t* relu_bits, const float* mask_h, const uint8_t* mask_b, float* zero_out, uint32_t* amax_out, int32_t mode,
                             int32_t* launched, void* stream) {
    GM_REQUIRE(b && x && W && out && K >= 1 && N >= 1 && ldx >= K && ldc >= N && mode >= -1 && mode <= 2 && !(mask_h && mask_b), GM_EINVAL,
               "dense_gemm: bad arguments");
    GM_REQUIRE(!amax_out || mode == 2, GM_EINVAL, "dense_gemm: amax_out is an output of the two-piece kernels (mode 2)");
    gm_gemm_args g{};
    g.A = x; g.lda = ldx; g.B = W; g.b_stride = w_stride; g.transB = trans_w ? 1 : 0; g.C = out; g.ldc = ldc; g.K = K; g.N = N;
    gemm_rows(g, scaled_level(b, s));
    gemm_keep_rows(g, RowView{s_keep}, s_keep != nullptr, false, b->rows);      // the caller's own keep vector
    g.bias = bias; g.bias_stride = bias_stride; g.relu = relu ? 1 : 0;
    g.relu_bits = relu_bits; g.mask_h = mask_h; g.mask_b = mask_b; g.zero_out = zero_out; g.amax_out = amax_out; g.launched = launched;
    const bool split = mode == 1 || mode == 2 || (mode < 0 && gm_gemm_split_ok(b->n_tiles, K, N));
    if (split) {
        GM_REQUIRE(!mask_h && !mask_b, GM_EINVAL, "dense_gemm: the split kernels take no relu' mask");
        GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 32, GM_EINVAL, "dense_gemm: the split kernels need N = 128 or 256 and K a multiple of 16 (>= 32)");
    }
    return launch_gemm(b, g, split, W, w_stride, trans_w ? 1 : 0, mode == 2 ? 2 : 3, x, ldx, true, "dense_gemm", (hipStream_t)stream);
}

// The fused aggregate + GEMM as fwd_update (model.hip) launches a fused layer: gm_dense_gemm with gm_gemm_args::fuse2 set.  The table is always the batch's own
// (table 0: d_fuse2 over the caller's x; 1: d_fuse2_feat over the batch's feature table), so the kernel reads no row outside its operands
// rowset -1: the batch's full tables (gm_dense_fused_gemm; s_keep: the caller's keep vector).  0 / 1 (gm_dense_fused_gemm_rows): the tables of the centre rows / of the
// sources of their in-edges through row_view, keep: the set's keep vector, live_on: its tile flags (2: and its packed tiles, GM_PACK_ROWS), grid workgroups (0: the production rule)
static int dense_fused_gemm(const gm_batch_t* b, int32_t rowset, int32_t keep, int32_t live_on, int32_t grid, int32_t table, const float* x, int64_t ldx, int32_t K, const float* zside, int64_t ldz,
                            const float* zfull, int64_t ldzf, const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc, const float* s,
                            const float* s_keep, const float* bias, int64_t bias_stride, int32_t relu, uint8_t* relu_bits, float* zero_out,
                            uint32_t* amax_out, int32_t mode, int32_t* launched, void* stream) {
    GM_REQUIRE(b && W && out && zside && K >= 1 && N >= 1 && ldz >= K && ldc >= N && (mode == 1 || mode == 2) && (table == 0 || table == 1), GM_EINVAL,
               "dense_fused_gemm: bad arguments");
    GM_REQUIRE(b->d_fuse2 && b->d_fuse2_feat, GM_EINVAL, "dense_fused_gemm: the batch carries no source tables");
    GM_REQUIRE(table == 1 || (x && ldx >= K), GM_EINVAL, "dense_fused_gemm: table 0 needs x and ldx >= K");
    GM_REQUIRE(table == 0 || (b->feat && (K == b->feat_dim || K == b->feat_ld)), GM_EINVAL, "dense_fused_gemm: table 1 needs K == feat_dim (%d)", b->feat_dim);
    GM_REQUIRE(!amax_out || mode == 2, GM_EINVAL, "dense_fused_gemm: amax_out is an output of the two-piece kernels (mode 2)");
    GM_REQUIRE(mode != 2 || (zfull && ldzf >= K), GM_EINVAL, "dense_fused_gemm: mode 2 takes its A bounds over a fully aggregated Z (zfull)");
    GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 32, GM_EINVAL, "dense_fused_gemm: the split kernels need N = 128 or 256 and K a multiple of 16 (>= 32)");
    gm_gemm_args g{};
    g.B = W; g.b_stride = w_stride; g.C = out; g.ldc = ldc; g.K = K; g.N = N;
    gemm_rows(g, scaled_level(b, s));
    gemm_keep_rows(g, RowView{s_keep}, s_keep != nullptr, false, b->rows);      // the caller's own keep vector
    g.bias = bias; g.bias_stride = bias_stride; g.relu = relu ? 1 : 0;
    g.relu_bits = relu_bits; g.zero_out = zero_out; g.amax_out = amax_out; g.launched = launched;
    g.zside = zside; g.ldz = ldz;
    if (table == 1) { g.A = b->feat; g.lda = b->feat_ld; } else { g.A = x; g.lda = ldx; }
    RowSet rs = ROWS_ALL;
    if (rowset >= 0) {
        GM_REQUIRE(rowset <= 1 && !(rowset == 0 && table == 1) && grid >= 0, GM_EINVAL, "dense_fused_gemm_rows: bad row set");
        GM_REQUIRE(b->d_fwd_tab[0] && b->d_fwd_tab[1] && b->d_fwd_tab_feat && b->d_tile_live[0] && b->d_tile_live[1], GM_EINVAL, "dense_fused_gemm_rows: the batch carries no row-set tables");
        rs = rowset == 0 ? ROWS_CENTRE : ROWS_E1;
        GM_REQUIRE(live_on != 2 || row_view(b, rs, false).pack, GM_EINVAL, "dense_fused_gemm_packed: the batch carries no packed row sets");
        gemm_keep_rows(g, row_view(b, rs, false), keep != 0, live_on != 0, b->rows, live_on == 2);
        g.grid_test = grid;
    }
    g.fuse2 = row_view(b, rs, table == 1).tab;
    // mode 2: per-set bounds of the rows the kernel forms, taken over the caller's fully aggregated Z -- never over zside, whose rows of one or two sources nobody
    // wrote --, and one per weight matrix: gm_dense_gemm's over a stored Z
    return launch_gemm(b, g, true, W, w_stride, 0, mode == 2 ? 2 : 3, zfull, ldzf, true, "dense_fused_gemm", (hipStream_t)stream);
}

extern "C" int gm_dense_fused_gemm(const gm_batch_t* b, int32_t table, const float* x, int64_t ldx, int32_t K, const float* zside, int64_t ldz,
                                   const float* zfull, int64_t ldzf, const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc, const float* s,
                                   const float* s_keep, const float* bias, int64_t bias_stride, int32_t relu, uint8_t* relu_bits, float* zero_out,
                                   uint32_t* amax_out, int32_t mode, int32_t* launched, void* stream) {
    return dense_fused_gemm(b, -1, 0, 0, 0, table, x, ldx, K, zside, ldz, zfull, ldzf, W, w_stride, N, out, ldc, s, s_keep, bias, bias_stride, relu, relu_bits, zero_out, amax_out,
                            mode, launched, stream);
}
// ... over the table of a row set, as the restricted forward-only layers launch it (GM_DEAD_ROWS=3, GM_DEAD_TILES; tests): rowset 0 the centre rows (gm_batch::d_fwd_tab[0],
// keep vector d_norm_c), 1 the sources of their in-edges (d_fwd_tab[1] / d_fwd_tab_feat, d_norm_e1).  keep: the set's keep vector is the launch's row_scale_keep (0: the
// batch's norm scales and every row is stored).  live_on: the launch gets the set's tile flags.  grid: workgroups (0: the production rule)
extern "C" int gm_dense_fused_gemm_rows(const gm_batch_t* b, int32_t rowset, int32_t keep, int32_t live_on, int32_t grid, int32_t table, const float* x, int64_t ldx, int32_t K,
                                        const float* zside, int64_t ldz, const float* zfull, int64_t ldzf, const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc,
                                        const float* bias, int64_t bias_stride, int32_t relu, uint8_t* relu_bits, float* zero_out, uint32_t* amax_out, int32_t mode,
                                        int32_t* launched, void* stream) {
    GM_REQUIRE(b && (rowset == 0 || rowset == 1) && b->d_norm_c && b->d_norm_e1, GM_EINVAL, "dense_fused_gemm_rows: bad arguments");
    return dense_fused_gemm(b, rowset, keep, live_on, grid, table, x, ldx, K, zside, ldz, zfull, ldzf, W, w_stride, N, out, ldc, b->d_norm, nullptr,
                            bias, bias_stride, relu, relu_bits, zero_out, amax_out, mode, launched, stream);
}

// ... over the row set's PACKED tiles, as the same layers launch it under GM_PACK_ROWS (tests): the set's keep vector, its tile flags and its packed tables
// (gm_batch::pack), three-piece kernel, grid workgroups (0: the production rule)
extern "C" int gm_dense_fused_gemm_packed(const gm_batch_t* b, int32_t rowset, int32_t grid, int32_t table, const float* x, int64_t ldx, int32_t K, const float* zside, int64_t ldz,
                                          const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc, const float* bias, int64_t bias_stride, int32_t relu,
                                          int32_t* launched, void* stream) {
    GM_REQUIRE(b && (rowset == 0 || rowset == 1) && b->d_norm_c && b->d_norm_e1, GM_EINVAL, "dense_fused_gemm_packed: bad arguments");
    return dense_fused_gemm(b, rowset, 1, 2, grid, table, x, ldx, K, zside, ldz, nullptr, 0, W, w_stride, N, out, ldc, b->d_norm, nullptr,
                            bias, bias_stride, relu, nullptr, nullptr, nullptr, 1, launched, stream);
}

// The dZ product of the last layer over a dQ that holds its centre rows only, as bwd_dz (model.hip) launches it under GM_DEAD_ROWS (tests)
extern "C" int gm_dense_dz_centre(const gm_batch_t* b, const float* dQ, int32_t K, const float* W, int64_t w_stride, int32_t N, float* T, void* stream) {
    GM_REQUIRE(b && dQ && W && T && b->d_dq_tab, GM_EINVAL, "dense_dz_centre: bad arguments");
    GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 64, GM_EINVAL, "dense_dz_centre: the fused split kernel needs N = 128 or 256 and K a multiple of 16 (>= 64)");
    gm_gemm_args g{};
    g.A = dQ; g.lda = K; g.B = W; g.b_stride = w_stride; g.transB = 1; g.C = T; g.ldc = N; g.K = K; g.N = N; g.np = 3;
    gemm_rows(g, batch_level(b)); gemm_dq_table(g, b, dQ, K);
    return launch_gemm(b, g, true, W, w_stride, 1, 3, nullptr, 0, false, "dense_dz_centre", (hipStream_t)stream);
}

// ... storing T's centre rows only, as bwd_dz launches it under GM_DEAD_ROWS=2 and up with the centres' tile flags (GM_DEAD_TILES); pack != 0: over the centres' packed
// tiles (GM_PACK_ROWS).  grid workgroups (0: the production rule)
extern "C" int gm_dense_dz_centre_rows(const gm_batch_t* b, const float* dQ, int32_t K, const float* W, int64_t w_stride, int32_t N, float* T, int32_t pack, int32_t grid, void* stream) {
    GM_REQUIRE(b && dQ && W && T && b->d_dq_tab && b->d_norm_c && b->d_tile_live[0] && grid >= 0, GM_EINVAL, "dense_dz_centre_rows: bad arguments");
    GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 64, GM_EINVAL, "dense_dz_centre_rows: the fused split kernel needs N = 128 or 256 and K a multiple of 16 (>= 64)");
    const RowView v = row_view(b, ROWS_CENTRE, false);
    GM_REQUIRE(!pack || v.pack, GM_EINVAL, "dense_dz_centre_rows: the batch carries no packed row sets");
    gm_gemm_args g{};
    g.A = dQ; g.lda = K; g.B = W; g.b_stride = w_stride; g.transB = 1; g.C = T; g.ldc = N; g.K = K; g.N = N; g.np = 3;
    gemm_rows(g, batch_level(b)); gemm_dq_table(g, b, dQ, K);
    gemm_keep_rows(g, v, true, true, b->n_c, pack != 0);
    g.grid_test = grid;
    return launch_gemm(b, g, true, W, w_stride, 1, 3, nullptr, 0, false, "dense_dz_centre_rows", (hipStream_t)stream);
}

// GM_DEAD_ROWS=2 (tests): the last layer's transposed aggregate dQ_prev = relu' norm A^T T as bwd_agg_t (model.hip) launches it.  keep != 0: T read through the batch's
// per-edge table (gm_batch::d_ect; T holds rows + 1 rows, the last one zeroed HERE) and only the rows gm_batch::d_norm_e1 keeps stored; keep == 0: the plain
// launch, every row of T read and every row of `out` stored.  mask_b: packed relu' bits [rows * width / 4], or NULL
extern "C" int gm_dense_agg_centre_t(const gm_batch_t* b, float* T, int32_t width, const uint8_t* mask_b, float* out, int32_t keep, void* stream) {
    GM_REQUIRE(b && T && out && width >= 4 && width % 4 == 0, GM_EINVAL, "dense_agg_centre_t: bad arguments");
    GM_REQUIRE(!keep || (b->d_ect && b->d_norm_e1), GM_EINVAL, "dense_agg_centre_t: the batch carries no centre-edge tables");
    hipStream_t st = (hipStream_t)stream;
    gm_agg_args a; GM_TRY(batch_agg(b, 1, 0, st, a));
    a.x = T; a.ldx = width; a.s_out = b->d_norm; a.mask_b = mask_b; a.out = out; a.width = width;
    if (keep) {
        GM_HIP(hipMemsetAsync(T + b->rows * (int64_t)width, 0, sizeof(float) * GM_ZERO_ROWS * width, st));
        agg_centre_t(a, b, ROWS_E1);
    }
    const int rc = gm_launch_aggregate(a, st);
    gm_batch_mark_use(b, st);
    return rc;
}

// ================================================================================ weight gradient, exported for numerics tests
// The scaffolding of the weight-gradient exports over rows v (the batch's; the export's own row scale): the partials; np == 2: two fp16 pieces per operand, marked by
// per-set bound slots of A (slots [0, sets)) and of G (slots [sets, 2 sets)) -- bounds: taken here over each set's rows (with the padding between them), and ONE bound
// of |a_scale| over all rows (slot 2 sets) as the gain of A's: |s x| <= max_t |x| * max |s|; else left zero (the launcher refuses two pieces with a table before any bound
// is read).  The launch, the frees
static int launch_wgrad(const gm_batch* b, gm_wgrad_args& w, const LevelView& v, int np, bool bounds, const char* who, hipStream_t st) {
    const int sets = b->sets;
    wgrad_rows(w, v);
    unsigned* slots = nullptr;
    int rc = gm_alloc(&w.partial, (size_t)std::max(1, b->n_chunks) * (size_t)((int64_t)w.K * w.N + w.N), st);
    if (rc == GM_OK && np == 2) {
        unsigned* sg = nullptr; unsigned* ss = nullptr;
        rc = gm_alloc(&slots, (size_t)(2 * sets + 1) * GM_BOUND_PAD, st);
        if (rc == GM_OK) { sg = slots + (int64_t)sets * GM_BOUND_PAD; ss = slots + (int64_t)2 * sets * GM_BOUND_PAD; }
        if (rc == GM_OK && hipMemsetAsync(slots, 0, sizeof(unsigned) * (2 * sets + 1) * GM_BOUND_PAD, st) != hipSuccess) { gm_set_error("%s: memset failed", who); rc = GM_EHIP; }
        if (rc == GM_OK && bounds) rc = set_row_amax(b, w.A, w.lda, w.K, slots, st);
        if (rc == GM_OK && bounds) rc = set_row_amax(b, w.G, w.ldg, w.N, sg, st);
        if (rc == GM_OK && bounds && w.a_scale) rc = gm_amax(w.a_scale, 0, 0, b->rows, 1, ss, 0, st);
        w.np = 2;
        w.a_bound = gm_no_bound(); w.a_bound.amax = slots; w.a_bound.stride = GM_BOUND_PAD;
        if (bounds && w.a_scale) w.a_bound.gain = reinterpret_cast<const float*>(ss);     // (an amax slot holds fp32 bits)
        w.g_bound = gm_no_bound(); w.g_bound.amax = sg; w.g_bound.stride = GM_BOUND_PAD;
    }
    if (rc == GM_OK) rc = gm_launch_wgrad(w, st);
    if (w.partial) gm_dev_free(w.partial, st);
    if (slots) gm_dev_free(slots, st);
    gm_batch_mark_use(b, st);
    return rc;
}

extern "C" int gm_dense_wgrad(const gm_batch_t* b, const float* x, int64_t ldx, int32_t K, const float* g, int64_t ldg, int32_t N, const float* s,
                              const float* gb, int64_t ldgb, float* dW, int64_t dw_stride, float* db, int64_t db_stride, int32_t mode,
                              const float* cur, float* next, int64_t p_stride, float lr, float* wt, uint16_t* pl_fwd, uint16_t* pl_dz, void* stream) {
    GM_REQUIRE(b && x && g && dW && K >= 1 && N >= 1 && ldx >= K && ldg >= N && (!gb || ldgb >= N) && mode >= -1 && mode <= 2, GM_EINVAL,
               "dense_wgrad: bad arguments");
    // the generic kernel's bias sums hold 2048 columns (bsum[2] x 1024 threads), and gm_make_layout stops there too
    GM_REQUIRE(K <= 2048 && N <= 2048, GM_ERANGE, "dense_wgrad: K=%d N=%d: at most 2048 columns per operand", K, N);
    const int sets = b->sets;
    const int64_t KN = (int64_t)K * N;
    GM_REQUIRE(sets == 1 || (dw_stride >= KN && (!db || db_stride >= N)), GM_EINVAL, "dense_wgrad: per-set outputs overlap");
    GM_REQUIRE(!next || (cur && db && (sets == 1 || p_stride >= KN + N)), GM_EINVAL, "dense_wgrad: the SGD step needs cur, db and a stride of at least (K+1)*N");
    GM_REQUIRE((!wt && !pl_fwd && !pl_dz) || next, GM_EINVAL, "dense_wgrad: wt and the planes are outputs of the SGD step");
    GM_REQUIRE((!pl_fwd && !pl_dz) || (K % 32 == 0 && N % 32 == 0), GM_EINVAL, "dense_wgrad: weight planes need K and N multiples of 32");
    gm_wgrad_args w{};
    w.A = x; w.lda = ldx; w.K = K; w.G = g; w.ldg = ldg; w.N = N; w.Gb = gb; w.ldgb = ldgb;
    w.dW = dW; w.dw_stride = dw_stride; w.db = db; w.db_stride = db_stride;
    if (next) {
        w.sgd_cur = cur; w.sgd_cur_stride = p_stride; w.sgd_next = next; w.sgd_next_stride = p_stride; w.sgd_lr = lr; w.w_off = 0; w.b_off = KN;
        w.wt_next = wt; w.pl_fwd = pl_fwd; w.pl_dz = pl_dz;
    }
    w.pick = mode == 0 ? GM_WGRAD_PICK_EXACT : mode > 0 ? GM_WGRAD_PICK_SPLIT : 0;
    return launch_wgrad(b, w, scaled_level(b, s), mode == 2 ? 2 : 3, true, "dense_wgrad", (hipStream_t)stream);
}

// The weight gradient over a Z whose forward ran fused, as bwd_wgrad_operands (model.hip) sets it up for a fused layer (LayerPlan::fuse): A holds the rows the table flags
// GM_FUSE_SELF, every other row is formed from gx through the batch's own table (table 0: d_fuse2 over the caller's gx; 1: d_fuse2_feat over the batch's feature table)
extern "C" int gm_dense_wgrad_fused(const gm_batch_t* b, int32_t table, const float* A, int64_t lda, int32_t K, const float* gx, int64_t ldgx, const float* g,
                                    int64_t ldg, int32_t N, const float* s, const float* g_keep, float* dW, int64_t dw_stride, float* db, int64_t db_stride,
                                    int32_t mode, void* stream) {
    GM_REQUIRE(b && A && g && dW && db && K >= 1 && N >= 1 && lda >= K && ldg >= N && mode >= 0 && mode <= 2 && (table == 0 || table == 1), GM_EINVAL,
               "dense_wgrad_fused: bad arguments");
    GM_REQUIRE(K <= 2048 && N <= 2048, GM_ERANGE, "dense_wgrad_fused: K=%d N=%d: at most 2048 columns per operand", K, N);
    GM_REQUIRE(b->d_fuse2 && b->d_fuse2_feat, GM_EINVAL, "dense_wgrad_fused: the batch carries no source tables");
    GM_REQUIRE(table == 1 || (gx && ldgx >= K), GM_EINVAL, "dense_wgrad_fused: table 0 needs gx and ldgx >= K");
    GM_REQUIRE(table == 0 || (b->feat && (K == b->feat_dim || K == b->feat_ld)), GM_EINVAL, "dense_wgrad_fused: table 1 needs K == feat_dim (%d)", b->feat_dim);
    GM_REQUIRE(b->sets == 1 || (dw_stride >= (int64_t)K * N && db_stride >= N), GM_EINVAL, "dense_wgrad_fused: per-set outputs overlap");
    gm_wgrad_args w{};
    w.A = A; w.lda = lda; w.K = K; w.G = g; w.ldg = ldg; w.N = N; w.g_keep = g_keep;
    w.dW = dW; w.dw_stride = dw_stride; w.db = db; w.db_stride = db_stride;
    w.fuse2 = row_view(b, ROWS_ALL, table == 1).tab;
    w.gx = table == 1 ? b->feat : gx; w.ldgx = table == 1 ? b->feat_ld : ldgx;
    w.pick = mode == 0 ? GM_WGRAD_PICK_EXACT : GM_WGRAD_PICK_SPLIT;
    return launch_wgrad(b, w, scaled_level(b, s), mode == 2 ? 2 : 3, false, "dense_wgrad_fused", (hipStream_t)stream);
}

// The weight gradients of a restricted backward (GM_DEAD_ROWS; tests): G = a dQ of which only the rows of a set were written -- the set's keep vector flags the others,
// which enter as zeros whatever their bytes hold.  _centre: dQ_L on its centre rows; _e1: dQ_{L-1} on the sources of the centres' in-edges
static int dense_wgrad_keep(const gm_batch_t* b, RowSet rs, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                            int64_t db_stride, void* stream) {
    GM_REQUIRE(b && x && dQ && dW && db && row_view(b, rs, false).keep, GM_EINVAL, "dense_wgrad_centre / _e1: bad arguments");
    GM_REQUIRE(b->sets == 1 || (dw_stride >= (int64_t)Kx * N && db_stride >= N), GM_EINVAL, "dense_wgrad_centre / _e1: per-set outputs overlap");
    gm_wgrad_args w{};
    w.A = x; w.lda = Kx; w.K = Kx; w.G = dQ; w.ldg = N; w.N = N; w.g_keep = row_view(b, rs, false).keep;
    w.dW = dW; w.dw_stride = dw_stride; w.db = db; w.db_stride = db_stride; w.pick = GM_WGRAD_PICK_SPLIT;
    return launch_wgrad(b, w, batch_level(b), 3, false, "dense_wgrad_centre / _e1", (hipStream_t)stream);
}
extern "C" int gm_dense_wgrad_centre(const gm_batch_t* b, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                                     int64_t db_stride, void* stream) {
    return dense_wgrad_keep(b, ROWS_CENTRE, x, Kx, dQ, N, dW, dw_stride, db, db_stride, stream);
}
extern "C" int gm_dense_wgrad_e1(const gm_batch_t* b, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                                 int64_t db_stride, void* stream) {
    return dense_wgrad_keep(b, ROWS_E1, x, Kx, dQ, N, dW, dw_stride, db, db_stride, stream);
}

// ================================================================================ aggregate, exported for numerics tests
// One launch of gm_launch_aggregate over one orientation of the batch with every field the production callers (gm_aggregate; fwd_mul_first, fwd_aggregate, bwd_mul_first,
// bwd_agg_t of model.hip) set, and the instantiation that ran (include/gmeta_hip.h)
extern "C" int gm_dense_aggregate(const gm_batch_t* b, int32_t transposed, int32_t x_src, const float* x, int64_t ldx, int32_t width, int32_t scale_src,
                                  const float* s_in, const float* s_out, int32_t keep_signed, const float* bias, int64_t bias_stride, int32_t relu,
                                  uint8_t* relu_bits, const float* mask_h, const uint8_t* mask_b, int32_t hubs, const int32_t* rowlist, int64_t n_list,
                                  int32_t list_win, int32_t list_sched, int32_t skip_lo, int32_t skip_hi, int32_t stream_ok, float* out, int32_t* launched,
                                  void* stream) {
    GM_REQUIRE(b && out && width >= 1 && x_src >= 0 && x_src <= 3 && scale_src >= 0 && scale_src <= 2 && hubs >= 0 && hubs <= 2, GM_EINVAL, "dense_aggregate: bad arguments");
    GM_REQUIRE(!(mask_h && mask_b), GM_EINVAL, "dense_aggregate: mask_h together with mask_b");
    GM_REQUIRE(!(rowlist && stream_ok), GM_EINVAL, "dense_aggregate: a row list together with the stream kernel");
    GM_REQUIRE(!stream_ok || hubs == 2, GM_EINVAL, "dense_aggregate: the stream kernel takes the batch's hub tables (hubs == 2)");
    const int o = transposed ? 1 : 0;
    const bool gather = x_src == 1 || x_src == 2;
    GM_REQUIRE(gather || (x && ldx >= width), GM_EINVAL, "dense_aggregate: a caller matrix needs x and ldx >= width");
    GM_REQUIRE(!gather || width == b->feat_dim, GM_EINVAL, "dense_aggregate: a gather needs width == feat_dim (%d)", b->feat_dim);
    GM_REQUIRE(x_src != 2 || (!transposed && b->d_efeat), GM_EINVAL, "dense_aggregate: the per-edge feature rows belong to the by-destination CSR");
    GM_REQUIRE(x_src != 3 || (transposed && b->d_ect), GM_EINVAL, "dense_aggregate: the centre-edge table belongs to the by-source CSR of a batch that carries one");
    GM_REQUIRE((scale_src == 1) == (s_in != nullptr), GM_EINVAL, "dense_aggregate: s_in goes with scale_src == 1 and only with it");
    GM_REQUIRE(scale_src != 2 || b->d_enorm[o], GM_EINVAL, "dense_aggregate: the batch has no per-edge norm table");
    GM_REQUIRE(!bias || !bias_stride || b->d_set_row_off, GM_EINVAL, "dense_aggregate: per-set bias without set row offsets");
    GM_REQUIRE(!keep_signed || s_out, GM_EINVAL, "dense_aggregate: keep_signed needs s_out");
    GM_REQUIRE(!relu_bits || relu, GM_EINVAL, "dense_aggregate: relu_bits are written with relu");
    // weighted batches, as gm_aggregate: only the per-edge tables have a slot for the edges' weights
    GM_REQUIRE(!b->weighted || scale_src != 1, GM_EINVAL, "dense_aggregate: on a weighted batch the source scale is none or the batch's own table (the per-source gather has no edge-weight slot)");
    // ... and a feature gather meets the weights only through the per-edge row table (gm_aggregate always takes it; the by-source CSR has none)
    GM_REQUIRE(!b->weighted || x_src != 1, GM_EINVAL, "dense_aggregate: on a weighted batch the feature gather goes through the per-edge row table (x_src 2; the per-source gather has no edge-weight slot)");
    hipStream_t st = (hipStream_t)stream;
    // the orientation as production's launches take it (agg_graph: an aggregate without a source scale carries a weighted batch's edge weights), hubs == 2: with its
    // block schedule and hub set (batch_agg); 1: the hub-row list alone; 0: not even that
    gm_agg_args a;
    if (hubs == 2) GM_TRY(batch_agg(b, o, 0, st, a)); else agg_graph(b, o, a);
    if (!hubs) { a.heavy = nullptr; a.n_heavy = 0; a.heavy_deg = 0; }
    a.width = width; a.out = out; a.launched = launched;
    if (gather) { a.x = b->feat; a.ldx = b->feat_ld; a.x_row = b->d_feat_row; if (x_src == 2) a.x_idx = b->d_efeat; }
    else { a.x = x; a.ldx = ldx; if (x_src == 3) agg_centre_t(a, b, ROWS_ALL); }
    if (scale_src == 1) a.s_in = s_in;
    if (scale_src == 2) { a.s_in = b->d_norm; a.e_w = b->d_enorm[o]; }
    a.s_out = s_out; a.keep_signed = keep_signed ? 1 : 0;
    a.bias = bias; a.bias_stride = bias_stride; a.set_row_off = b->d_set_row_off; a.n_sets = b->sets;
    a.relu = relu ? 1 : 0; a.relu_bits = relu_bits; a.mask_h = mask_h; a.mask_b = mask_b;
    if (skip_lo <= skip_hi) { a.skip_on = 1; a.skip_lo = skip_lo; a.skip_hi = skip_hi; }
    if (rowlist) {
        GM_REQUIRE(n_list >= 1 && n_list <= b->rows && list_win >= 2 && list_win <= 64 && (list_win & (list_win - 1)) == 0, GM_EINVAL,
                   "dense_aggregate: a row list needs 1 .. rows entries and a window of 2, 4, .. 64 rows");
        std::vector<int32_t> h((size_t)n_list);
        GM_HIP(hipMemcpyAsync(h.data(), rowlist, sizeof(int32_t) * (size_t)n_list, hipMemcpyDeviceToHost, st));
        GM_HIP(hipStreamSynchronize(st));
        for (int64_t k = 0; k < n_list; ++k)
            GM_REQUIRE(h[k] >= 0 && h[k] < b->rows && (k == 0 || h[k] > h[k - 1]), GM_EINVAL, "dense_aggregate: the row list is not ascending / out of range at entry %lld", (long long)k);
        a.rowlist = rowlist; a.n_list = n_list; a.list_win = list_win;
        if (list_sched) {
            // the batch's block schedule over its own list of window rows (fwd_aggregate's partial launch of a fused layer)
            GM_REQUIRE(hubs == 2 && !transposed && b->d_sched_mid && n_list == b->n_mid && list_win == b->mid_win, GM_EINVAL,
                       "dense_aggregate: the list schedule goes with the batch's own list (%d rows, windows of %d) and its hub tables", b->n_mid, b->mid_win);
            a.sched = b->d_sched_mid; a.sched_len = b->sched_len_mid; a.sched_win = b->mid_win;
        } else { a.sched = nullptr; a.sched_len = 0; }
    } else if (list_sched >= 2 && list_sched <= 4) {
        // one of the batch's own lists of observable rows (gm_batch::obs[list_sched - 2]) as fwd_aggregate / bwd_agg_t (model.hip) launch over it (agg_take_list): the list at its bound, its
        // window, the length the device counted and, where the orientation has hub rows, the list's own schedule.  Built or not taken by the batch: both allowed here
        const gm_batch::obs_list& ol = b->obs[list_sched - 2];
        GM_REQUIRE(ol.rows && (list_sched == 4) == (transposed != 0), GM_EINVAL, "dense_aggregate: the batch holds no list %d of this orientation", list_sched - 2);
        GM_REQUIRE(ol.cap >= 1 || ol.sched, GM_EINVAL, "dense_aggregate: list %d is empty and the orientation has no hub rows: nothing to launch", list_sched - 2);
        GM_REQUIRE(b->n_heavy[o] == 0 || (hubs == 2 && ol.sched), GM_EINVAL, "dense_aggregate: list %d has no schedule for the orientation's hub rows", list_sched - 2);
        agg_take_list(a, ol);
    } else GM_REQUIRE(!list_sched, GM_EINVAL, "dense_aggregate: a list schedule without a row list");
    if (stream_ok && a.e_w && a.e_w == b->d_enorm[o]) GM_TRY(gm_agg_stream_args(a, b, o, gather, st));
    const int rc = gm_launch_aggregate(a, st);
    gm_batch_mark_use(b, st);
    return rc;
}

// What the tests of gm_dense_aggregate need to know about orientation o of a batch: info[16] = {hub threshold, hub rows, rows per scheduled window, edges
// per hub part (0: unsplit), hub parts, scheduled (0 / 1), rows of the batch's window-row list, its window, list schedule (0 / 1), stream row segments (0 until the
// orientation's first stream-eligible launch), stream workgroups, hub workgroups among them, weighted, feat_dim, feat_ld, 0}.  (Sixteen entries for good: callers
// hold exactly that many.)
extern "C" int gm_dense_agg_info(const gm_batch_t* b, int32_t transposed, int64_t* info) {
    GM_REQUIRE(b && info, GM_EINVAL, "dense_agg_info: bad arguments");
    const int o = transposed ? 1 : 0;
    const int64_t v[16] = {b->heavy_deg, b->n_heavy[o], b->sched_win, b->hub_part[o], b->hub_parts[o], b->d_sched[o] ? 1 : 0, b->d_mid ? b->n_mid : 0, b->mid_win,
                           b->d_sched_mid ? 1 : 0, b->d_sseg[o] ? b->stream_nseg[o] : 0, b->stream_nwg[o], b->stream_hubwg[o], b->weighted ? 1 : 0, b->feat_dim, b->feat_ld, 0};
    std::copy(v, v + 16, info);
    return GM_OK;
}
// The batch's lists of observable rows (gm_batch::obs; GM_AGG_OBS_LIST), four entries per list k = 0, 1, 2: info[4 k ..] = {length (read back from the device at first
// use, which synchronises the stream; 0 where the list was not built), bound it was allocated and scheduled for, rows per window, how the batch takes it (0 today's
// launch, 1 the list, 2 nothing to launch) + 4 where it carries a block schedule}; info[12 .. 15] = {gm_batch_fwd_counts(0)[0], gm_batch_fwd_counts(1)[0] (the observable rows
// of more than GM_FUSE_MAXDEG sources, hub rows included; -1 without the forward-only tables), gm_batch_e1_rows, 0}: what the lengths are checked against
extern "C" int gm_dense_obs_lists(const gm_batch_t* b, int64_t* info, void* stream) {
    GM_REQUIRE(b && info, GM_EINVAL, "dense_obs_lists: bad arguments");
    for (int k = 0; k < 3; ++k) {
        const gm_batch::obs_list& ol = b->obs[k];
        if (ol.n < 0) {
            int32_t h = 0;
            if (ol.rows && ol.len) { GM_HIP(hipMemcpyAsync(&h, ol.len, 4, hipMemcpyDeviceToHost, (hipStream_t)stream)); GM_HIP(hipStreamSynchronize((hipStream_t)stream)); }
            ol.n = h;
        }
        info[4 * k] = ol.n; info[4 * k + 1] = ol.cap; info[4 * k + 2] = ol.win; info[4 * k + 3] = ol.take + (ol.sched ? 4 : 0);
    }
    for (int k = 0; k < 2; ++k) {
        int64_t w[3] = {-1, -1, -1};
        if (b->d_obs[k] && b->rows > 0) GM_TRY(gm_batch_fwd_counts(b, k, (hipStream_t)stream, w));
        info[12 + k] = w[0];
    }
    info[14] = gm_batch_e1_rows(b, (hipStream_t)stream); info[15] = 0;
    gm_batch_mark_use(b, (hipStream_t)stream);
    return GM_OK;
}
// ... and the tests of the fused kernels: counts[2] = {rows of more than GM_FUSE_MAXDEG sources (gm_batch::unfused_rows: the rows a fused pass still aggregates by
// the ordinary kernel), their in-edges (unfused_edges)}
extern "C" int gm_dense_fuse_counts(const gm_batch_t* b, int64_t* counts) {
    GM_REQUIRE(b && counts, GM_EINVAL, "dense_fuse_counts: bad arguments");
    counts[0] = b->unfused_rows; counts[1] = b->unfused_edges;
    return GM_OK;
}
// Device copies of the batch's derived tables (which: 0 per-edge source norm of orientation o [edges] float, 1 per-edge feature row [edges] int32, 2 window-row
// list [info[6]] int32, 3 hub rows of orientation o [info[1]] int32; 4 / 5 / 6 the per-row source tables gm_batch::d_fuse2 / d_fuse2_feat / d_dq_tab, [rows] entries
// of four int32 {u0, u1, w0, w1}; 7 / 8 / 9 the forward-only passes' tables of GM_DEAD_ROWS=3 in the same layout: the last layer's (gm_batch::d_fwd_tab[0]), the layer
// below it over batch rows (d_fwd_tab[1]) and over the feature table (d_fwd_tab_feat); 10 / 11 / 12 the lists of observable rows gm_batch::obs[0 .. 2], int32; 13 / 14 the tile flags
// gm_batch::d_tile_live[0 / 1], one int32 per GEMM row tile; 15 / 16 the packed row ids of the centre rows / of the sources of their in-edges (gm_batch::pack[0 / 1].rowid,
// up to the host's bound), 17 / 18 their packed tile tables ({set, offset, nrows}: n counts int32 words, up to three per tile of the bound), 19 / 20 their tile counts
// (one int32)): n entries -> dst (device)
extern "C" int gm_dense_agg_table(const gm_batch_t* b, int32_t which, int32_t transposed, void* dst, int64_t n, void* stream) {
    GM_REQUIRE(b && dst && n >= 0 && which >= 0 && which <= 20, GM_EINVAL, "dense_agg_table: bad arguments");
    if (which >= 15) {      // 15 .. 20: the packed row sets (gm_batch::pack)
        const gm_batch::pack_set& pk = b->pack[(which - 15) & 1];
        const int kind = (which - 15) >> 1;
        const int32_t* src = kind == 0 ? pk.rowid : kind == 1 ? pk.tiles : pk.count;
        const int64_t have = !pk.tiles ? 0 : kind == 0 ? pk.cap_rows : kind == 1 ? 3 * (int64_t)pk.cap_tiles : 1;
        GM_REQUIRE(pk.tiles && src && n <= have, GM_EINVAL, "dense_agg_table: table %d holds %lld entries", which, (long long)have);
        if (n) GM_HIP(hipMemcpyAsync(dst, src, 4 * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        gm_batch_mark_use(b, (hipStream_t)stream);
        return GM_OK;
    }
    if (which >= 13) {      // 13 / 14: the tile flags of the centre rows / of the sources of their in-edges (gm_batch::d_tile_live), one int32 per GEMM row tile
        const int32_t* fl = b->d_tile_live[which - 13];
        GM_REQUIRE(fl && n <= b->n_tiles, GM_EINVAL, "dense_agg_table: table %d holds %lld entries", which, (long long)(fl ? b->n_tiles : 0));
        if (n) GM_HIP(hipMemcpyAsync(dst, fl, 4 * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        gm_batch_mark_use(b, (hipStream_t)stream);
        return GM_OK;
    }
    if (which >= 10) {      // 10 / 11 / 12: the lists of observable rows (gm_dense_obs_lists), up to their bound
        const gm_batch::obs_list& ol = b->obs[which - 10];
        GM_REQUIRE(ol.rows && n <= ol.cap, GM_EINVAL, "dense_agg_table: table %d holds %lld entries", which, (long long)(ol.rows ? ol.cap : 0));
        if (n) GM_HIP(hipMemcpyAsync(dst, ol.rows, 4 * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        gm_batch_mark_use(b, (hipStream_t)stream);
        return GM_OK;
    }
    const int o = transposed ? 1 : 0;
    const void* src = which == 0 ? (const void*)b->d_enorm[o] : which == 1 ? (const void*)b->d_efeat : which == 2 ? (const void*)b->d_mid : which == 3 ? (const void*)b->d_heavy[o]
                    : which == 4 ? (const void*)b->d_fuse2 : which == 5 ? (const void*)b->d_fuse2_feat : which == 6 ? (const void*)b->d_dq_tab
                    : which == 7 ? (const void*)b->d_fwd_tab[0] : which == 8 ? (const void*)b->d_fwd_tab[1] : (const void*)b->d_fwd_tab_feat;
    const int64_t have = which <= 1 ? b->edges : which == 2 ? b->n_mid : which == 3 ? b->n_heavy[o] : b->rows;
    GM_REQUIRE(src && n <= have, GM_EINVAL, "dense_agg_table: table %d holds %lld entries", which, (long long)(src ? have : 0));
    if (n) GM_HIP(hipMemcpyAsync(dst, src, (which >= 4 ? 16 : 4) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    gm_batch_mark_use(b, (hipStream_t)stream);
    return GM_OK;
}
