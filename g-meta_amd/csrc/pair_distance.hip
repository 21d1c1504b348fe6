// Shortest-path distances of sources and node pairs (gm_store_node_distances, gm_store_pair_distance: graph distance, the oldest of the link-prediction
// baselines).  The DEFINITION is in include/gmeta_hip.h; tests/distance_ref.py restates it with a plain breadth-first search.  This file is how it is computed,
// over the neighbour index (nbr_index.hip; gm_nbr.h):
//   columns     a column is a pair (s, x): the search from s in the graph without the edge {s, x} (x = -1: the whole graph).  The host reads the sources or pairs
//               back once, forms the DISTINCT columns in ascending (s, x) order (gm_columns.h) and runs them in rounds of at most B
//               (gm_set_tuning("dist_cols")); with the mask flag only adjacent pairs get a column of their own.  The call's frame -- knob checks, read-back
//               and plan, adjacency, hub cut -- is gm_columns.h.
//   the state   ONE BIT per (node, column): three bit matrices [N, W] of 64-bit words, W = B / 64 -- seen, frontier, next.  A level is a pull over the symmetric
//               rows: next[v] = (OR over z in G(v) of frontier[z]) & ~seen[v], seen[v] |= next[v]; frontier and next swap.  Every word of the three is written by
//               exactly one lane with a plain vector store (seen[v] is read by the lane that owns it alone); there are no atomics.
//   one row     a lane owns one word of a row.  A row is L lanes wide, L the power of two that holds W (a template parameter: 1 .. 64), and a wave takes 64 / L
//               rows; at B = 4096 a wave takes one row with a wave-uniform neighbour id and every neighbour costs one coalesced 512-byte row read.
//               GM_DIST_UNROLL row reads are in flight per lane.  A word whose columns are all seen (the padding columns of the last round count as seen)
//               issues no gathers.
//   levels end  changed[t] is set by the level that found a new bit; the kernels of level t + 1 and the result kernels of level t return at once when the flag
//               they read is 0, so the host enqueues max_dist levels without a round trip.  Every GM_DIST_SYNC_EVERY levels it reads the flag back and stops
//               enqueueing (one stream synchronisation per 16 levels: nothing at the default max_dist of 8, at most 15 of 254).
//   hub rows    a row of more than C entries (gm_set_tuning("dist_chunk")) is cut into segments of C: k_dist_parts ORs each segment into a partial buffer,
//               k_dist_hubs ORs the partials and finishes the row.  OR is associative and commutative: no cut can change a bit.
//   the mask    needs no test per neighbour.  CLAIM: the levels of the column (s, x), x in G(s), in G' = G without {s, x} are the levels in G after the bit of
//               the column is cleared in next[x] and seen[x] behind level 1.  PROOF: the two graphs differ in the rows of s and x alone: G(s) = G'(s) + {x},
//               G(x) = G'(x) + {s}.  Level 0 is {s} in both.  Level 1 pulls from the frontier {s}: in G it is G(s), in G' it is G(s) - {x}; x is not s, so
//               clearing x's bit in next and seen gives the state of G' exactly.  At a level t >= 2 the extra entry x of row s is read by row s alone, whose
//               bit has been seen since level 0 and is masked by ~seen whatever the OR gives; the extra entry s of row x contributes frontier[s], which is
//               0 from level 1 on (s is in the frontier at level 0 only).  So from level 2 on both graphs give the same next for every row, by induction.
//               The host lists one (word, bit mask) item per distinct (x, word) of a round, so k_dist_unmask's threads own their words too.
//   results     gm_store_pair_distance: k_dist_probe tests the target bit of every pair in next behind each level and stores the level where it is set (it is
//               set at one level only: seen).  gm_store_node_distances: d_out is prefilled with 255; behind each level k_dist_rows_out turns the new bits
//               into bytes: a workgroup per (64 nodes, one word of 64 columns), a lane keeps its node's word in a register and a wave per output row of
//               those columns stores the level where the bit is set -- 64 consecutive bytes of one row of d_out per wave store, with no transpose through
//               LDS (the word IS the transposed tile).  A column serves every duplicate of its source.
//   scratch     3 N W 8 bytes of state (W = min(B, columns rounded up to 64) / 64: 3 N B / 8), 8 W bytes per hub segment, 4 (max_dist + 1) bytes of flags
//               and the lists of the columns, hub segments and output entries (4 .. 16 bytes each), from the stream-ordered pool.
//   profiles    gm_store_pair_distance_profile (at the end of the file) counts, per pair, the nodes a hops from one endpoint and b hops from the other: a third
//               emit on dist_rounds.  Both columns of a pair must be alive in one round, so the pairs are cut into groups of at most Bp distinct columns
//               (gm_columns.h: gm_col_pair_groups) and every group is a plan and a single round of its own.  Behind each level the new bits are transposed
//               into node-major planes, behind the last a wave per pair counts on them (distance_profile.hip); only [n, D + 2, D + 2] integers leave the
//               device.  Scratch beside the search's: (D + 1) Bp ceil(N / 64) 8 bytes of planes (gm_set_tuning("dist_plane_kib") bounds Bp) and 16 bytes per pair.
// A result is a function of (graph, source or pair, flags, max_dist) alone.  Everything runs on the caller's stream.
#include "gm_columns.h"

#define GM_DIST_THREADS 256
#define GM_DIST_UNROLL 8                  // row reads of the frontier in flight per lane
#define GM_DIST_MAX_COLS 4096             // W <= 64: a row is never wider than a wave
#define GM_DIST_SYNC_EVERY 16             // levels between two read-backs of the flag

// the columns of word w that do not exist (a round holds n_live columns): they count as seen
__device__ __forceinline__ uint64_t dist_dead(int32_t w, int32_t n_live) {
    const int32_t k = n_live - w * 64;
    return k >= 64 ? 0ull : k <= 0 ? ~0ull : ~0ull << k;
}

// OR over row[0 .. len) of F[z, w] (Fw = F + w)
__device__ __forceinline__ uint64_t dist_or(const int32_t* __restrict__ row, int32_t len, const uint64_t* __restrict__ Fw, int64_t W) {
    uint64_t acc = 0;
    int32_t i = 0;
    for (; i + GM_DIST_UNROLL <= len; i += GM_DIST_UNROLL) {
        int32_t z[GM_DIST_UNROLL]; uint64_t q[GM_DIST_UNROLL];
#pragma unroll
        for (int k = 0; k < GM_DIST_UNROLL; ++k) z[k] = row[i + k];
#pragma unroll
        for (int k = 0; k < GM_DIST_UNROLL; ++k) q[k] = Fw[(int64_t)z[k] * W];
#pragma unroll
        for (int k = 0; k < GM_DIST_UNROLL; ++k) acc |= q[k];
    }
    for (; i < len; ++i) acc |= Fw[(int64_t)row[i] * W];
    return acc;
}

// the new bits of a word: stored to next, added to seen
__device__ __forceinline__ uint64_t dist_store(uint64_t acc, uint64_t sn, int64_t at, uint64_t* __restrict__ next, uint64_t* __restrict__ seen) {
    const uint64_t nx = acc & ~sn;
    next[at] = nx;
    if (nx) seen[at] = sn | nx;
    return nx;
}

// seen = the columns that do not exist, frontier = 0: a thread per word
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_init(int64_t words, int32_t W, int32_t n_live, uint64_t* __restrict__ seen, uint64_t* __restrict__ cur) {
    const int64_t i = (int64_t)blockIdx.x * GM_DIST_THREADS + threadIdx.x;
    if (i >= words) return;
    seen[i] = dist_dead((int32_t)(i % W), n_live);
    cur[i] = 0;
}

// level 0: the bit of every column on its source's row.  A thread per word of columns: the columns ascend by source, so the columns of one source inside a
// word are consecutive and the thread stores their bits with one store per (source, word) -- words of different threads differ
__global__ void __launch_bounds__(GM_WAVE) k_dist_seed(const int32_t* __restrict__ cs, int32_t W, int32_t n_live, uint64_t* __restrict__ seen, uint64_t* __restrict__ cur,
                                                       int32_t* __restrict__ changed) {
    const int32_t w = (int32_t)threadIdx.x;
    if (w == 0) changed[0] = 1;
    if (w >= W) return;
    const uint64_t dead = dist_dead(w, n_live);
    int32_t prev = -1;
    uint64_t m = 0;
    for (int b = 0; b <= 64; ++b) {
        const int32_t s = b < 64 && w * 64 + b < n_live ? cs[w * 64 + b] : -1;
        if (s != prev) {
            if (prev >= 0) { cur[(int64_t)prev * W + w] = m; seen[(int64_t)prev * W + w] = dead | m; }
            prev = s; m = 0;
        }
        m |= b < 64 ? 1ull << b : 0ull;
    }
}

// a group of L lanes per row, a lane per word; rows of more than C entries are left to k_dist_parts / k_dist_hubs.  flag[0]: the level before found a bit;
// flag[1]: this one did
template <int L>
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_rows(gm_nbr_graph G, int32_t W, int32_t C, int32_t* __restrict__ flag, const uint64_t* __restrict__ F,
                                                               uint64_t* __restrict__ next, uint64_t* __restrict__ seen) {
    if (flag[0] == 0) return;
    const int64_t t = (int64_t)blockIdx.x * GM_DIST_THREADS + threadIdx.x;
    const int64_t row = t / L;
    const int32_t w = (int32_t)(t & (L - 1));
    uint64_t nx = 0;
    if (row < G.N && w < W) {
        const int32_t v = L == GM_WAVE ? __builtin_amdgcn_readfirstlane((int32_t)row) : (int32_t)row;
        const int64_t r0 = G.ptr[v];
        const int64_t deg = G.ptr[v + 1] - r0;
        if (deg <= C) {
            const int64_t at = (int64_t)v * W + w;
            const uint64_t sn = seen[at];
            bool need = ~sn != 0;
            if (L == GM_WAVE) need = __any(need);                                  // (the wave's row: the loop and its neighbour ids stay wave-uniform)
            nx = dist_store(need ? dist_or(G.idx + r0, (int32_t)deg, F + w, W) : 0ull, sn, at, next, seen);
        }
    }
    if (__syncthreads_or(nx != 0) && threadIdx.x == 0) flag[1] = 1;
}

// a group per segment of a hub row: part[item, w] = the segment's OR
template <int L>
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_parts(gm_nbr_graph G, int32_t W, int32_t C, const int32_t* __restrict__ flag, const int32_t* __restrict__ it_row,
                                                                const int32_t* __restrict__ it_seg, int64_t n_items, const uint64_t* __restrict__ F,
                                                                const uint64_t* __restrict__ seen, uint64_t* __restrict__ part) {
    if (flag[0] == 0) return;
    const int64_t t = (int64_t)blockIdx.x * GM_DIST_THREADS + threadIdx.x;
    const int64_t item = t / L;
    const int32_t w = (int32_t)(t & (L - 1));
    if (item >= n_items || w >= W) return;
    const int32_t it = L == GM_WAVE ? __builtin_amdgcn_readfirstlane((int32_t)item) : (int32_t)item;
    const int32_t v = it_row[it];
    const int64_t r0 = G.ptr[v], beg = (int64_t)it_seg[it] * C;
    const int64_t left = G.ptr[v + 1] - r0 - beg;
    const int32_t len = (int32_t)(left < C ? left : C);
    bool need = ~seen[(int64_t)v * W + w] != 0;
    if (L == GM_WAVE) need = __any(need);
    part[(int64_t)it * W + w] = need ? dist_or(G.idx + r0 + beg, len, F + w, W) : 0ull;
}

// a group per hub row: the OR of its partials, then the row as k_dist_rows finishes it
template <int L>
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_hubs(int32_t W, int32_t* __restrict__ flag, const int32_t* __restrict__ hub_row, const int32_t* __restrict__ hub_first,
                                                               int64_t n_hubs, const uint64_t* __restrict__ part, uint64_t* __restrict__ next, uint64_t* __restrict__ seen) {
    if (flag[0] == 0) return;
    const int64_t t = (int64_t)blockIdx.x * GM_DIST_THREADS + threadIdx.x;
    const int64_t hub = t / L;
    const int32_t w = (int32_t)(t & (L - 1));
    uint64_t nx = 0;
    if (hub < n_hubs && w < W) {
        const int32_t v = hub_row[hub], first = hub_first[hub], segs = hub_first[hub + 1] - first;
        uint64_t acc = 0;
        for (int32_t k = 0; k < segs; ++k) acc |= part[(int64_t)(first + k) * W + w];
        const int64_t at = (int64_t)v * W + w;
        nx = dist_store(acc, seen[at], at, next, seen);
    }
    if (__syncthreads_or(nx != 0) && threadIdx.x == 0) flag[1] = 1;
}

// behind level 1: the masked columns lose their bit on the row of their excluded node (the proof is in the header comment); a thread per (node, word) item
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_unmask(const int64_t* __restrict__ at, const uint64_t* __restrict__ bits, int64_t cnt, uint64_t* __restrict__ next,
                                                                 uint64_t* __restrict__ seen) {
    const int64_t i = (int64_t)blockIdx.x * GM_DIST_THREADS + threadIdx.x;
    if (i >= cnt) return;
    const uint64_t keep = ~bits[i];
    next[at[i]] &= keep; seen[at[i]] &= keep;
}

// gm_store_pair_distance: out[dst[e]] = level where next holds the bit (node[e], col[e] - c0), for the cnt entries of a round
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_probe(const uint64_t* __restrict__ next, int32_t W, int64_t c0, const int32_t* __restrict__ flag, const int64_t* __restrict__ dst,
                                                                const int32_t* __restrict__ node, const int32_t* __restrict__ col, int64_t cnt, int32_t level, uint8_t* __restrict__ out) {
    if (flag[0] == 0) return;
    const int64_t e = (int64_t)blockIdx.x * GM_DIST_THREADS + threadIdx.x;
    if (e >= cnt) return;
    const int64_t c = (int64_t)col[e] - c0;
    if ((next[(int64_t)node[e] * W + (c >> 6)] >> (c & 63)) & 1) out[dst[e]] = (uint8_t)level;
}

// gm_store_node_distances: out[row[r], v] = level where next holds the bit (v, col[r] - c0), for the cnt output rows of a round (col ascending).  A workgroup
// per (64 nodes, word w): lanes are nodes, a wave per output row whose column lies in the word
__global__ void __launch_bounds__(GM_DIST_THREADS) k_dist_rows_out(const uint64_t* __restrict__ next, int32_t W, int64_t c0, int64_t N, const int32_t* __restrict__ flag,
                                                                   const int32_t* __restrict__ row, const int32_t* __restrict__ col, int64_t cnt, int32_t level, uint8_t* __restrict__ out) {
    if (flag[0] == 0) return;
    const int32_t w = (int32_t)(blockIdx.x % (unsigned)W);
    const int64_t v = (int64_t)(blockIdx.x / (unsigned)W) * GM_WAVE + (threadIdx.x & (GM_WAVE - 1));
    const uint64_t bits = v < N ? next[v * W + w] : 0ull;
    if (!__any(bits != 0)) return;
    const int64_t first = c0 + (int64_t)w * 64;
    int64_t lo = 0, hi = cnt;                                                  // the first output row whose column is at least `first`
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (col[mid] < first) lo = mid + 1; else hi = mid;
    }
    for (int64_t r = lo + (threadIdx.x >> 6); r < cnt; r += GM_DIST_THREADS / GM_WAVE) {
        const int64_t b = (int64_t)col[r] - first;
        if (b >= 64) break;
        if ((bits >> b) & 1) out[(int64_t)row[r] * N + v] = (uint8_t)level;
    }
}

// Columns per round and entries per hub segment, from the sweep at the arxiv shape (profiles/pair_distance.txt).  The widest round wins wherever there are
// columns to fill it -- a level costs its launches and the longest row's tail once per round (4,096 sources: 22.7 / 9.1 / 6.0 / 5.5 ms at 64 / 256 / 1,024 /
// 4,096 columns) --, so the library takes the bound; a round is never wider than the call's columns.  The cut: segments of 64 .. 256 lie within a few percent of
// each other and 128 is the fastest or within 2 % of it on every row; uncut rows (the longest has 2,648 entries) cost up to 1.7 x on the narrow calls, whose
// levels wait for that one row (64 sources: 0.60 ms at 128 against 1.01 uncut), and 4 % on the widest.
static int dist_cols_for() { return GM_DIST_MAX_COLS; }
static int32_t dist_chunk_for() { return 128; }

static unsigned dist_grid(int64_t threads) { return (unsigned)((threads + GM_DIST_THREADS - 1) / GM_DIST_THREADS); }

struct dist_call : gm_col_call { int32_t max_dist; };

// the checks both exports share; n == 0 leaves c->B == 0 (nothing to do)
static int dist_begin(const char* what, const char* cnt_name, const gm_store* s, int32_t g, int64_t n, int32_t flags, int32_t max_dist, const void* d_in, const void* d_out,
                      void* stream, dist_call* c) {
    GM_TRY(gm_store_call_check(what, s, g, cnt_name, n, flags));
    GM_REQUIRE(max_dist >= 1 && max_dist <= 254, GM_EINVAL, "%s: max_dist = %d; 1 .. 254", what, max_dist);
    c->max_dist = max_dist;
    return gm_col_setup(what, {gm_knob().dist_cols, "dist_cols", gm_knob().dist_chunk, "dist_chunk", GM_DIST_MAX_COLS, dist_cols_for(), dist_chunk_for()}, s, g, n, d_in, d_out, stream,
                        c);
}

// one level of a round, F -> next: the rows up to C entries, then the hub rows' segments and the hub rows.  flag: changed + (level - 1)
template <int L>
static void dist_level(const dist_call& c, int32_t W, const gm_col_hubs<uint64_t>& H, int32_t* flag, const uint64_t* F, uint64_t* next, uint64_t* seen) {
    const dim3 block(GM_DIST_THREADS);
    hipLaunchKernelGGL(k_dist_rows<L>, dim3(dist_grid(c.G.N * L)), block, 0, c.st, c.G, W, c.C, flag, F, next, seen);
    if (!H.n_hubs) return;
    hipLaunchKernelGGL(k_dist_parts<L>, dim3(dist_grid(H.n_items * L)), block, 0, c.st, c.G, W, c.C, (const int32_t*)flag, (const int32_t*)H.it_row, (const int32_t*)H.it_seg, H.n_items, F,
                       (const uint64_t*)seen, H.part);
    hipLaunchKernelGGL(k_dist_hubs<L>, dim3(dist_grid(H.n_hubs * L)), block, 0, c.st, W, flag, (const int32_t*)H.row, (const int32_t*)H.first, H.n_hubs, (const uint64_t*)H.part, next, seen);
}
typedef void (*dist_level_fn)(const dist_call&, int32_t, const gm_col_hubs<uint64_t>&, int32_t*, const uint64_t*, uint64_t*, uint64_t*);
// the instantiation whose group of lanes holds the W words of a row
static dist_level_fn dist_level_for(int32_t W) {
    return W <= 1 ? dist_level<1> : W <= 2 ? dist_level<2> : W <= 4 ? dist_level<4> : W <= 8 ? dist_level<8> : W <= 16 ? dist_level<16> : W <= 32 ? dist_level<32> : dist_level<64>;
}

// The search of the plan's columns (cs[k], cx[k]), ascending, in rounds of at most B: behind every level t = 0 .. max_dist of a round emit(t, c0, Br, next, flag)
// reads the level's new bits next[N, Br / 64] of the columns c0 .. c0 + Br on the call's stream; flag[0] == 0 on the device says that the level found none.
template <class Emit>
static int dist_rounds(const char* what, const dist_call& c, const gm_col_plan& pl, gm_stager& sg, Emit emit) {
    const gm_nbr_graph& G = c.G;
    const std::vector<int32_t>& cs = pl.cs;
    const std::vector<int32_t>& cx = pl.cx;
    const int64_t N = G.N, ncols = (int64_t)cs.size(), ncp = (ncols + GM_WAVE - 1) / GM_WAVE * GM_WAVE;
    if (!ncols) return GM_OK;
    const int64_t Bmax = ncp < c.B ? ncp : c.B, Wmax = Bmax / GM_WAVE;
    GM_REQUIRE(N * GM_WAVE / GM_DIST_THREADS < (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld nodes pass the launch's 2^31 workgroups", what, (long long)N);
    gm_col_hub_lists hl;
    GM_TRY(gm_col_hub_cut(what, pl.h_ptr, N, c.C, 25, "dist_chunk", &hl));     // (INT32_MAX / GM_WAVE segments)
    gm_col_hubs<uint64_t> H;
    // the (word, bits) items k_dist_unmask clears behind level 1, round by round: one item per distinct (excluded node, word)
    std::vector<int64_t> un_at, un_first;
    std::vector<uint64_t> un_bits;
    for (int64_t c0 = 0; c0 < ncp; c0 += c.B) {
        const int64_t Br = ncp - c0 < c.B ? ncp - c0 : c.B, Wr = Br / GM_WAVE, end = c0 + Br < ncols ? c0 + Br : ncols;
        std::vector<std::pair<int64_t, uint64_t>> items;
        for (int64_t k = c0; k < end; ++k)
            if (cx[(size_t)k] >= 0) items.push_back({(int64_t)cx[(size_t)k] * Wr + (k - c0) / 64, 1ull << ((k - c0) & 63)});
        std::sort(items.begin(), items.end());
        un_first.push_back((int64_t)un_at.size());
        for (const auto& it : items) {
            if ((int64_t)un_at.size() > un_first.back() && un_at.back() == it.first) un_bits.back() |= it.second;
            else { un_at.push_back(it.first); un_bits.push_back(it.second); }
        }
    }
    un_first.push_back((int64_t)un_at.size());

    gm_scratch sc(c.st);
    uint64_t *seen = nullptr, *Fa = nullptr, *Fb = nullptr, *d_un_bits = nullptr;
    int64_t* d_un_at = nullptr;
    int32_t *d_cs = nullptr, *changed = nullptr;
    GM_TRY(sc.take(&seen, (size_t)(N * Wmax))); GM_TRY(sc.take(&Fa, (size_t)(N * Wmax))); GM_TRY(sc.take(&Fb, (size_t)(N * Wmax)));
    GM_TRY(sc.take(&changed, (size_t)(c.max_dist + 1)));
    GM_TRY(sc.put(&d_cs, cs, sg));
    GM_TRY(sc.put(&d_un_at, un_at, sg)); GM_TRY(sc.put(&d_un_bits, un_bits, sg));
    GM_TRY(gm_col_hubs_put(&H, hl, Wmax, sc, sg));
    const dim3 block(GM_DIST_THREADS);
    int64_t round = 0;
    for (int64_t c0 = 0; c0 < ncp; c0 += c.B, ++round) {
        const int32_t Br = (int32_t)(ncp - c0 < c.B ? ncp - c0 : c.B), W = Br / GM_WAVE;
        const int32_t n_live = (int32_t)(ncols - c0 < Br ? ncols - c0 : Br);
        const dist_level_fn level = dist_level_for(W);
        GM_HIP(hipMemsetAsync(changed, 0, (size_t)(c.max_dist + 1) * sizeof(int32_t), c.st));
        hipLaunchKernelGGL(k_dist_init, dim3(dist_grid(N * W)), block, 0, c.st, N * W, W, n_live, seen, Fa);
        hipLaunchKernelGGL(k_dist_seed, dim3(1), dim3(GM_WAVE), 0, c.st, (const int32_t*)d_cs + c0, W, n_live, seen, Fa, changed);
        GM_HIP(hipGetLastError());
        uint64_t *cur = Fa, *next = Fb;
        GM_TRY(emit(0, c0, Br, (const uint64_t*)cur, (const int32_t*)changed));
        for (int32_t t = 1; t <= c.max_dist; ++t) {
            level(c, W, H, changed + (t - 1), cur, next, seen);
            const int64_t un = un_first[(size_t)round + 1] - un_first[(size_t)round];
            if (t == 1 && un)
                hipLaunchKernelGGL(k_dist_unmask, dim3(dist_grid(un)), block, 0, c.st, (const int64_t*)d_un_at + un_first[(size_t)round], (const uint64_t*)d_un_bits + un_first[(size_t)round], un,
                                   next, seen);
            GM_HIP(hipGetLastError());
            GM_TRY(emit(t, c0, Br, (const uint64_t*)next, (const int32_t*)changed + t));
            std::swap(cur, next);
            if (t % GM_DIST_SYNC_EVERY == 0 && t < c.max_dist) {
                const int32_t* h = sg.download((const int32_t*)changed + t, 1);
                GM_REQUIRE(h, GM_ENOMEM, "%s: pinned staging allocation failed", what);
                GM_HIP(hipStreamSynchronize(c.st));
                if (!*h) break;
            }
        }
    }
    return GM_OK;
}

extern "C" int32_t gm_store_node_distances(const gm_store_t* s, int32_t g, const int32_t* d_sources, int64_t m, int32_t max_dist, uint8_t* d_out, void* stream) {
    const char* what = "gm_store_node_distances";
    dist_call c;
    GM_TRY(dist_begin(what, "m", s, g, m, 0, max_dist, d_sources, d_out, stream, &c));
    if (!c.B) return GM_OK;
    const int64_t N = c.G.N;
    gm_stager sg(c.st);
    gm_scratch sc(c.st);
    gm_col_plan pl;
    int32_t *d_row = nullptr, *d_col = nullptr;
    GM_HIP(hipMemsetAsync(d_out, GM_DIST_UNREACHED, (size_t)m * (size_t)N, c.st));      // (ahead of the plan's synchronisation)
    GM_TRY(gm_col_sources(what, c, d_sources, m, sg, sc, &pl, &d_row, &d_col));
    const int64_t v_tiles = (N + GM_WAVE - 1) / GM_WAVE;
    return dist_rounds(what, c, pl, sg, [&](int32_t t, int64_t c0, int32_t Br, const uint64_t* next, const int32_t* flag) {
        int64_t lo, hi;
        gm_col_span(pl.col, c0, Br, false, &lo, &hi);
        if (hi == lo) return (int)GM_OK;
        const int64_t blocks = v_tiles * (Br / GM_WAVE);
        GM_REQUIRE(blocks <= (int64_t)INT32_MAX, GM_ERANGE, "%s: %lld output tiles in one round", what, (long long)blocks);
        hipLaunchKernelGGL(k_dist_rows_out, dim3((unsigned)blocks), dim3(GM_DIST_THREADS), 0, c.st, next, Br / GM_WAVE, c0, N, flag, (const int32_t*)d_row + lo, (const int32_t*)d_col + lo,
                           hi - lo, t, d_out);
        GM_HIP(hipGetLastError());
        return (int)GM_OK;
    });
}

extern "C" int32_t gm_store_pair_distance(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, int32_t max_dist, uint8_t* d_out, void* stream) {
    const char* what = "gm_store_pair_distance";
    dist_call c;
    GM_TRY(dist_begin(what, "n", s, g, n, flags, max_dist, d_pairs, d_out, stream, &c));
    if (!c.B) return GM_OK;
    gm_scratch sc(c.st);
    gm_stager sg(c.st);
    gm_col_plan pl;                                                        // one entry per pair: the bit of v in the column of u
    int64_t* d_dst = nullptr;
    int32_t *d_node = nullptr, *d_col = nullptr;
    GM_HIP(hipMemsetAsync(d_out, GM_DIST_UNREACHED, (size_t)n, c.st));     // (ahead of the plan's synchronisation)
    GM_TRY(gm_col_pairs(what, c, d_pairs, n, (flags & GM_PAIR_MASK_TARGET) != 0, false, sg, sc, &pl, &d_dst, &d_node, &d_col));
    return dist_rounds(what, c, pl, sg, [&](int32_t t, int64_t c0, int32_t Br, const uint64_t* next, const int32_t* flag) {
        int64_t lo, hi;
        gm_col_span(pl.col, c0, Br, false, &lo, &hi);
        if (hi == lo) return (int)GM_OK;
        hipLaunchKernelGGL(k_dist_probe, dim3(dist_grid(hi - lo)), dim3(GM_DIST_THREADS), 0, c.st, next, Br / GM_WAVE, c0, flag, (const int64_t*)d_dst + lo, (const int32_t*)d_node + lo,
                           (const int32_t*)d_col + lo, hi - lo, t, d_out);
        GM_HIP(hipGetLastError());
        return (int)GM_OK;
    });
}

// ---- gm_store_pair_distance_profile: the third emit on dist_rounds (the planes and the count are distance_profile.hip)
#define GM_DIST_PROFILE_MAX 7             // max_dist of a profile: the range of gm_set_hop_labels, a table of at most 81 entries
#define GM_DIST_PLANE_KIB (1 << 20)       // the library's budget of level planes: 1 GiB

// GM_TIMING: the three phases of a call, the stream synchronised behind each (tools/distance_profile_bench.py reads the line)
struct dist_laps {
    bool on; hipStream_t st; double us[3] = {0, 0, 0};
    std::chrono::steady_clock::time_point t;
    explicit dist_laps(hipStream_t s) : on(gm_knob().timing != 0), st(s) { if (on) { (void)hipStreamSynchronize(st); t = std::chrono::steady_clock::now(); } }
    void lap(int phase) {
        if (!on) return;
        (void)hipStreamSynchronize(st);
        const auto n = std::chrono::steady_clock::now();
        us[phase] += std::chrono::duration<double, std::micro>(n - t).count();
        t = n;
    }
};

extern "C" int32_t gm_store_pair_distance_profile(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, int32_t max_dist, int32_t* d_out, void* stream) {
    const char* what = "gm_store_pair_distance_profile";
    GM_TRY(gm_store_call_check(what, s, g, "n", n, flags));
    GM_REQUIRE(max_dist >= 1 && max_dist <= GM_DIST_PROFILE_MAX, GM_EINVAL, "%s: max_dist = %d; 1 .. %d", what, max_dist, GM_DIST_PROFILE_MAX);
    const int kib = gm_knob().dist_plane_kib;
    GM_REQUIRE(kib >= 0, GM_EINVAL, "%s: dist_plane_kib = %d", what, kib);
    dist_call c;
    GM_TRY(dist_begin(what, "n", s, g, n, flags, max_dist, d_pairs, d_out, stream, &c));
    if (!c.B) return GM_OK;
    const int64_t N = c.G.N, NW = (N + GM_WAVE - 1) / GM_WAVE, L = max_dist + 1, E = (L + 1) * (L + 1);
    // the columns of a group: what the search holds in a round, and what the budget holds of planes
    const int64_t budget = (int64_t)(kib ? kib : GM_DIST_PLANE_KIB) * 1024, per_word = L * GM_WAVE * NW * (int64_t)sizeof(uint64_t);
    GM_REQUIRE(budget >= per_word, GM_ERANGE, "%s: the level planes of 64 columns take %lld bytes at N = %lld, max_dist = %d; dist_plane_kib = %d holds %lld", what,
               (long long)per_word, (long long)N, max_dist, kib ? kib : GM_DIST_PLANE_KIB, (long long)budget);
    const int64_t fit = budget / per_word * GM_WAVE, Bp = fit < c.B ? fit : c.B;
    gm_scratch sc(c.st);
    gm_stager sg(c.st);
    GM_HIP(hipMemsetAsync(d_out, 0, (size_t)n * (size_t)E * sizeof(int32_t), c.st));      // a pair with a node outside the graph (ahead of the read-back's synchronisation)
    gm_col_pairs_host R;
    GM_TRY(gm_col_pairs_read(what, c, d_pairs, n, (flags & GM_PAIR_MASK_TARGET) != 0, sg, sc, &R));
    gm_col_groups G;
    GM_TRY(gm_col_pair_groups(what, N, R, n, (flags & GM_PAIR_MASK_TARGET) != 0, Bp, &G));
    if (G.groups.empty()) return GM_OK;
    int64_t Bmax = 0;                                                          // the widest group, in whole words of columns
    for (const gm_col_group& gr : G.groups) {
        const int64_t b = ((int64_t)gr.plan.cs.size() + GM_WAVE - 1) / GM_WAVE * GM_WAVE;
        Bmax = b > Bmax ? b : Bmax;
    }
    uint64_t* T = nullptr;
    int64_t* d_dst = nullptr;
    int32_t *d_cu = nullptr, *d_cv = nullptr;
    GM_TRY(sc.take(&T, (size_t)(L * Bmax * NW)));
    GM_TRY(sc.put(&d_dst, G.dst, sg)); GM_TRY(sc.put(&d_cu, G.cu, sg)); GM_TRY(sc.put(&d_cv, G.cv, sg));
    dist_laps laps(c.st);
    int64_t cols_run = 0;                                                      // the columns searched, padding included: a column may serve pairs of several groups
    for (const gm_col_group& gr : G.groups) {
        const int64_t Bg = ((int64_t)gr.plan.cs.size() + GM_WAVE - 1) / GM_WAVE * GM_WAVE;      // one round: Bg <= Bp <= c.B
        GM_HIP(hipMemsetAsync(T, 0, (size_t)(L * Bg * NW) * sizeof(uint64_t), c.st));
        cols_run += Bg;
        GM_TRY(dist_rounds(what, c, gr.plan, sg, [&](int32_t t, int64_t c0, int32_t Br, const uint64_t* next, const int32_t* flag) {
            GM_REQUIRE(c0 == 0 && Br == Bg, GM_ERANGE, "%s: a group of %lld columns in more than one round", what, (long long)gr.plan.cs.size());
            laps.lap(0);
            GM_TRY(gm_prof_transpose(c.st, next, Br / GM_WAVE, N, flag, T + (int64_t)t * Bg * NW));
            laps.lap(1);
            return (int)GM_OK;
        }));
        laps.lap(0);
        GM_TRY(gm_prof_count(c.st, T, max_dist, Bg, N, (const int32_t*)d_cu + gr.first, (const int32_t*)d_cv + gr.first, (const int64_t*)d_dst + gr.first, gr.cnt, d_out));
        laps.lap(2);
    }
    if (laps.on)
        fprintf(stderr, "[gm timing] %s groups %lld columns %lld search %.1f us transpose %.1f us count %.1f us\n", what, (long long)G.groups.size(), (long long)cols_run, laps.us[0],
                laps.us[1], laps.us[2]);
    return GM_OK;
}
