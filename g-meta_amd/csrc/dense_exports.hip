// Single launches of the update GEMM, the dZ product and the weight gradient as gcn_forward / gcn_backward (model.hip) issue them.  Host code only.
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

// ================================================================================ dense update, exported for numerics tests
extern "C" int gm_dense_update(const gm_batch_t* b, const float* x, int32_t K, const float* W, int64_t w_stride, int32_t N, float* out, int32_t mode,
                               void* stream) {
    GM_REQUIRE(b && x && W && out && K >= 1 && N >= 1, GM_EINVAL, "dense_update: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    gm_gemm_args g{};
    g.A = x; g.lda = K; g.B = W; g.b_stride = w_stride; g.C = out; g.ldc = N; g.K = K; g.N = N;
    g.tiles = b->d_tiles; g.n_tiles = b->n_tiles; g.rows = b->rows;
    uint16_t* planes = nullptr; unsigned* slots = nullptr;
    const bool split = mode == 1 || mode == 2 || (mode < 0 && gm_gemm_split_ok(b->n_tiles, K, N));
    if (split) {
        GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 32, GM_EINVAL, "dense_update: the split kernels need N = 128 or 256 and K a multiple of 16 (>= 32)");
        const int sets = w_stride ? b->sets : 1;
        GM_TRY(gm_alloc(&planes, (size_t)sets * 3 * K * N, st));
        int rc = GM_OK;
        gm_bound wb = gm_no_bound();
        if (mode == 2) {
            // two fp16 pieces per operand: bounds taken here -- one for all of x (slot 0), one per weight matrix (slots 1..)
            rc = gm_alloc(&slots, (size_t)(sets + 1) * GM_BOUND_PAD, st);
            if (rc == GM_OK && hipMemsetAsync(slots, 0, sizeof(unsigned) * (sets + 1) * GM_BOUND_PAD, st) != hipSuccess) { gm_set_error("dense_update: memset failed"); rc = GM_EHIP; }
            if (rc == GM_OK) rc = gm_amax(x, 0, 0, (int64_t)b->rows * K, 1, slots, 0, st);
            if (rc == GM_OK) rc = gm_amax(W, w_stride, 0, (int64_t)K * N, sets, slots + GM_BOUND_PAD, GM_BOUND_PAD, st);
            wb.amax = slots + GM_BOUND_PAD; wb.stride = w_stride ? GM_BOUND_PAD : 0;
            g.np = 2; g.a_bound = gm_no_bound(); g.a_bound.amax = slots; g.b_bound = wb;
        }
        if (rc == GM_OK) rc = gm_split_weights(W, w_stride, 0, K, N, 0, sets, planes, st, mode == 2 ? 2 : 3, wb);
        if (rc != GM_OK) { gm_dev_free(planes, st); if (slots) gm_dev_free(slots, st); return rc; }
        g.Bsplit = planes; g.bsplit_stride = w_stride ? (int64_t)3 * K * N : 0;
    }
    const int rc = gm_launch_gemm_nn(g, st);
    if (planes) gm_dev_free(planes, st);
    if (slots) gm_dev_free(slots, st);
    gm_batch_mark_use(b, st);
    return rc;
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
    hipStream_t st = (hipStream_t)stream;
    const int sets = b->sets;
    gm_gemm_args g{};
    g.A = x; g.lda = ldx; g.B = W; g.b_stride = w_stride; g.transB = trans_w ? 1 : 0; g.C = out; g.ldc = ldc; g.K = K; g.N = N;
    g.row_scale = s; g.row_scale_keep = s_keep; g.n_keep = b->rows; g.bias = bias; g.bias_stride = bias_stride; g.relu = relu ? 1 : 0;
    g.relu_bits = relu_bits; g.mask_h = mask_h; g.mask_b = mask_b; g.zero_out = zero_out;
    g.tiles = b->d_tiles; g.n_tiles = b->n_tiles; g.rows = b->rows; g.launched = launched;
    uint16_t* planes = nullptr; unsigned* slots = nullptr;
    int rc = GM_OK;
    if (mode == 1 || mode == 2 || (mode < 0 && gm_gemm_split_ok(b->n_tiles, K, N))) {
        GM_REQUIRE(!mask_h && !mask_b, GM_EINVAL, "dense_gemm: the split kernels take no relu' mask");
        GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 32, GM_EINVAL, "dense_gemm: the split kernels need N = 128 or 256 and K a multiple of 16 (>= 32)");
        const int wsets = w_stride ? sets : 1;
        rc = gm_alloc(&planes, (size_t)wsets * 3 * K * N, st);
        gm_bound wb = gm_no_bound();
        if (rc == GM_OK && mode == 2) {
            // two fp16 pieces per operand: per-set bounds of x (slots [0, sets)), taken over each set's rows as gm_dense_wgrad does, and one per
            // weight matrix (slots [sets, sets + wsets))
            rc = gm_alloc(&slots, (size_t)(sets + wsets) * GM_BOUND_PAD, st);
            if (rc == GM_OK && hipMemsetAsync(slots, 0, sizeof(unsigned) * (sets + wsets) * GM_BOUND_PAD, st) != hipSuccess) { gm_set_error("dense_gemm: memset failed"); rc = GM_EHIP; }
            if (rc == GM_OK) rc = set_row_amax(b, x, ldx, K, slots, st);
            if (rc == GM_OK) rc = gm_amax(W, w_stride, 0, (int64_t)K * N, wsets, slots + (int64_t)sets * GM_BOUND_PAD, GM_BOUND_PAD, st);
            wb.amax = slots + (int64_t)sets * GM_BOUND_PAD; wb.stride = w_stride ? GM_BOUND_PAD : 0;
            g.np = 2; g.a_bound = gm_no_bound(); g.a_bound.amax = slots; g.a_bound.stride = GM_BOUND_PAD; g.b_bound = wb; g.amax_out = amax_out;
        }
        // trans_w: W stored [N, K] -- the planes are its own rows (as the dZ product's)
        if (rc == GM_OK) rc = gm_split_weights(W, w_stride, 0, K, N, trans_w ? 1 : 0, wsets, planes, st, mode == 2 ? 2 : 3, wb);
        g.Bsplit = planes; g.bsplit_stride = w_stride ? (int64_t)3 * K * N : 0;
    }
    if (rc == GM_OK) rc = gm_launch_gemm_nn(g, st);
    if (planes) gm_dev_free(planes, st);
    if (slots) gm_dev_free(slots, st);
    gm_batch_mark_use(b, st);
    return rc;
}

// The dZ product of the last layer over a dQ that holds its centre rows only, as gcn_backward launches it under GM_DEAD_ROWS (tests)
extern "C" int gm_dense_dz_centre(const gm_batch_t* b, const float* dQ, int32_t K, const float* W, int64_t w_stride, int32_t N, float* T, void* stream) {
    GM_REQUIRE(b && dQ && W && T && b->d_dq_tab, GM_EINVAL, "dense_dz_centre: bad arguments");
    GM_REQUIRE((N == 256 || N == 128) && K % 16 == 0 && K >= 64, GM_EINVAL, "dense_dz_centre: the fused split kernel needs N = 128 or 256 and K a multiple of 16 (>= 64)");
    hipStream_t st = (hipStream_t)stream;
    const int wsets = w_stride ? b->sets : 1;
    uint16_t* planes = nullptr;
    GM_TRY(gm_alloc(&planes, (size_t)wsets * 3 * K * N, st));
    gm_gemm_args g{};
    g.A = dQ; g.lda = K; g.B = W; g.b_stride = w_stride; g.transB = 1; g.C = T; g.ldc = N; g.K = K; g.N = N;
    g.row_scale = b->d_norm; g.tiles = b->d_tiles; g.n_tiles = b->n_tiles; g.rows = b->rows;
    g.fuse2 = b->d_dq_tab; g.zside = dQ; g.ldz = K;
    int rc = gm_split_weights(W, w_stride, 0, K, N, 1, wsets, planes, st, 3, gm_no_bound());
    g.Bsplit = planes; g.bsplit_stride = w_stride ? (int64_t)3 * K * N : 0; g.np = 3;
    if (rc == GM_OK) rc = gm_launch_gemm_nn(g, st);
    gm_dev_free(planes, st);
    gm_batch_mark_use(b, st);
    return rc;
}
// ... and its weight gradient (keep: the flagged row scale that says which rows of dQ were written)
static int dense_wgrad_keep(const gm_batch_t* b, const float* keep, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                            int64_t db_stride, void* stream) {
    GM_REQUIRE(b && x && dQ && dW && db && keep, GM_EINVAL, "dense_wgrad_centre / _e1: bad arguments");
    const int64_t KN = (int64_t)Kx * N;
    GM_REQUIRE(b->sets == 1 || (dw_stride >= KN && db_stride >= N), GM_EINVAL, "dense_wgrad_centre / _e1: per-set outputs overlap");
    hipStream_t st = (hipStream_t)stream;
    gm_wgrad_args w{};
    w.A = x; w.lda = Kx; w.K = Kx; w.G = dQ; w.ldg = N; w.N = N; w.a_scale = b->d_norm; w.g_keep = keep;
    w.chunks = b->d_chunks; w.n_chunks = b->n_chunks; w.set_chunk_off = b->d_set_chunk_off; w.sets = b->sets; w.rows = b->rows;
    w.dW = dW; w.dw_stride = dw_stride; w.db = db; w.db_stride = db_stride; w.pick = GM_WGRAD_PICK_SPLIT;
    int rc = gm_alloc(&w.partial, (size_t)std::max(1, b->n_chunks) * (size_t)(KN + N), st);
    if (rc == GM_OK) rc = gm_launch_wgrad(w, st);
    if (w.partial) gm_dev_free(w.partial, st);
    gm_batch_mark_use(b, st);
    return rc;
}
extern "C" int gm_dense_wgrad_centre(const gm_batch_t* b, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                                     int64_t db_stride, void* stream) {
    return dense_wgrad_keep(b, b ? b->d_norm_c : nullptr, x, Kx, dQ, N, dW, dw_stride, db, db_stride, stream);
}

// GM_DEAD_ROWS=2 (tests): the last layer's transposed aggregate dQ_prev = relu' norm A^T T as gcn_backward launches it.  keep != 0: T read through the batch's
// per-edge table (gm_batch::d_ect; T holds rows + 1 rows, the last one zeroed HERE) and only the rows gm_batch::d_norm_e1 keeps stored; keep == 0: the plain
// launch, every row of T read and every row of `out` stored.  mask_b: packed relu' bits [rows * width / 4], or NULL
extern "C" int gm_dense_agg_centre_t(const gm_batch_t* b, float* T, int32_t width, const uint8_t* mask_b, float* out, int32_t keep, void* stream) {
    GM_REQUIRE(b && T && out && width >= 4 && width % 4 == 0, GM_EINVAL, "dense_agg_centre_t: bad arguments");
    GM_REQUIRE(!keep || (b->d_ect && b->d_norm_e1), GM_EINVAL, "dense_agg_centre_t: the batch carries no centre-edge tables");
    hipStream_t st = (hipStream_t)stream;
    gm_agg_args a{};
    a.indptr = b->d_indptr_t; a.indices = b->d_indices_t;
    a.heavy = b->d_heavy[1]; a.n_heavy = b->n_heavy[1]; a.heavy_deg = b->heavy_deg;
    a.sched = b->d_sched[1]; a.sched_len = b->sched_len[1]; a.sched_win = b->sched_win;
    GM_TRY(gm_agg_hub(a, b, 1, st));
    if (b->weighted) a.e_w = b->d_ew[1];
    a.rows = b->rows; a.x = T; a.ldx = width; a.s_out = b->d_norm; a.mask_b = mask_b; a.out = out; a.width = width;
    if (keep) {
        GM_HIP(hipMemsetAsync(T + b->rows * (int64_t)width, 0, sizeof(float) * GM_ZERO_ROWS * width, st));
        a.x_idx = b->d_ect; a.s_out = b->d_norm_e1; a.keep_signed = 1;
    }
    const int rc = gm_launch_aggregate(a, st);
    gm_batch_mark_use(b, st);
    return rc;
}
// ... and the weight gradient of the layer below over that dQ_prev: rows gm_batch::d_norm_e1 flags enter as zeros, whatever their bytes hold
extern "C" int gm_dense_wgrad_e1(const gm_batch_t* b, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                                 int64_t db_stride, void* stream) {
    return dense_wgrad_keep(b, b ? b->d_norm_e1 : nullptr, x, Kx, dQ, N, dW, dw_stride, db, db_stride, stream);
}

// ================================================================================ weight gradient, exported for numerics tests
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
    hipStream_t st = (hipStream_t)stream;
    gm_wgrad_args w{};
    w.A = x; w.lda = ldx; w.K = K; w.G = g; w.ldg = ldg; w.N = N; w.Gb = gb; w.ldgb = ldgb; w.a_scale = s;
    w.chunks = b->d_chunks; w.n_chunks = b->n_chunks; w.set_chunk_off = b->d_set_chunk_off; w.sets = sets; w.rows = b->rows;
    w.dW = dW; w.dw_stride = dw_stride; w.db = db; w.db_stride = db_stride;
    if (next) {
        w.sgd_cur = cur; w.sgd_cur_stride = p_stride; w.sgd_next = next; w.sgd_next_stride = p_stride; w.sgd_lr = lr; w.w_off = 0; w.b_off = KN;
        w.wt_next = wt; w.pl_fwd = pl_fwd; w.pl_dz = pl_dz;
    }
    w.pick = mode == 0 ? GM_WGRAD_PICK_EXACT : mode > 0 ? GM_WGRAD_PICK_SPLIT : 0;
    unsigned* slots = nullptr;
    int rc = gm_alloc(&w.partial, (size_t)std::max(1, b->n_chunks) * (size_t)(KN + N), st);
    if (rc == GM_OK && mode == 2) {
        // two fp16 pieces per operand: per-set bounds of x (slots [0, sets)) and of g (slots [sets, 2 sets)), taken over each set's rows (with
        // the padding between them), and ONE bound of |s| over all rows (slot 2 sets) as the gain of x's: |s x| <= max_t |x| * max |s|
        rc = gm_alloc(&slots, (size_t)(2 * sets + 1) * GM_BOUND_PAD, st);
        if (rc == GM_OK && hipMemsetAsync(slots, 0, sizeof(unsigned) * (2 * sets + 1) * GM_BOUND_PAD, st) != hipSuccess) { gm_set_error("dense_wgrad: memset failed"); rc = GM_EHIP; }
        if (rc == GM_OK) rc = set_row_amax(b, x, ldx, K, slots, st);
        if (rc == GM_OK) rc = set_row_amax(b, g, ldg, N, slots + (int64_t)sets * GM_BOUND_PAD, st);
        if (rc == GM_OK && s) rc = gm_amax(s, 0, 0, b->rows, 1, slots + (int64_t)2 * sets * GM_BOUND_PAD, 0, st);
        w.np = 2;
        w.a_bound = gm_no_bound(); w.a_bound.amax = slots; w.a_bound.stride = GM_BOUND_PAD;
        if (s) w.a_bound.gain = reinterpret_cast<const float*>(slots + (int64_t)2 * sets * GM_BOUND_PAD);     // (an amax slot holds fp32 bits)
        w.g_bound = gm_no_bound(); w.g_bound.amax = slots + (int64_t)sets * GM_BOUND_PAD; w.g_bound.stride = GM_BOUND_PAD;
    }
    if (rc == GM_OK) rc = gm_launch_wgrad(w, st);
    if (w.partial) gm_dev_free(w.partial, st);
    if (slots) gm_dev_free(slots, st);
    gm_batch_mark_use(b, st);
    return rc;
}
