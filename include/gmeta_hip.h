/* gmeta_hip.h -- C ABI of libgmeta_hip.so: the MI355X (gfx950) implementation of G-Meta's
 * inner-loop hot path.  Plain pointers and sizes only; no torch types.
 *
 * The reference (mims-harvard/G-Meta) is pure Python and has no FFI layer: its boundary is the
 * Python call surface Subgraphs.__getitem__/collate -> Meta.forward/finetunning ->
 * Classifier.forward, with all native work delegated to the third-party DGL 0.4.3 + torch 1.5.
 * Each entry point below names the reference code it replaces (paths relative to
 * /root/reference/G-Meta/).  The Python host mirror in g-meta_amd/ binds these through ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: every function returns GM_OK (0) or a negative GM_E* code; gm_last_error()
 * returns a thread-local message for the last failure.  `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  Pointers documented "device" are HBM addresses on the
 * current HIP device; "host" are ordinary host pointers.  Handles (gm_store_t, gm_batch_t) own
 * their HBM and are released by the matching *_destroy; workspaces are caller-provided.
 * A handle is not thread-safe; distinct handles may be used from distinct threads.
 */
#ifndef GMETA_HIP_H
#define GMETA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GM_OK 0
#define GM_EINVAL (-1)  /* bad argument (also: update_step < 2, unequal class counts)      */
#define GM_ENOMEM (-2)  /* HBM / workspace too small                                      */
#define GM_EHIP (-3)    /* a HIP runtime call failed                                      */
#define GM_ERANGE (-4)  /* size outside what the kernels support (e.g. a batch above 2^31 rows) */
#define GM_MAX_GCN 4

typedef struct gm_store gm_store_t; /* parent graphs (in/out CSR) + node features, resident in HBM */
typedef struct gm_batch gm_batch_t; /* a batched set of induced subgraphs (one or many task sets)   */

typedef struct gm_seed { int32_t graph, i, j; } gm_seed_t; /* j = -1 for node classification */

/* Model description == the `config` list built at train.py:67-75:
 * [('GraphConv',[dims[0],dims[1]]), ..., ('Linear',[dims[n_gcn], n_out])] (+('LinkPred',[True])).
 * Parameter vector layout (== Classifier.vars order, learner.py:81-97), flat fp32:
 *   W_1[dims0 x dims1] row-major [in,out], b_1[dims1], ..., W_lin[n_out x (dims[n_gcn]*(1+link_pred))], b_lin[n_out] */
typedef struct gm_model {
    int32_t n_gcn;
    int32_t dims[GM_MAX_GCN + 1];
    int32_t n_out;
    int32_t link_pred;
} gm_model_t;

/* Hyper-parameters read by Meta.__init__ (meta.py:85-92). */
typedef struct gm_hparams {
    float update_lr;       /* args.update_lr                                            */
    int32_t update_step;   /* K: args.update_step (train) or args.update_step_test      */
    int32_t k_spt;         /* n_support of proto_loss_spt (meta.py:123)                 */
    int32_t need_meta_grad;/* 1 = Meta.forward (meta.py:101-173), 0 = finetunning (175-234) */
    int32_t hoist_z1;      /* 0 = reference-equivalent schedule (every forward re-aggregates layer 1);
                              1 = aggregate layer-1 input once per call (loop-invariant)   */
    int32_t serialize;     /* 0 = support chain and query evaluations on two HIP streams (default);
                              1 = everything on `stream` (for per-kernel timing / profiling)  */
    int32_t sparse_bwd;    /* 0 = dense backward over every subgraph row (reference-equivalent schedule, default);
                              1 = exact row-sparse backward: only the head touches the last layer, so dQ_L is non-zero
                              at centre rows only and dQ_{L-1} only along in-edges of centres -- same sums without
                              the structural zeros (models with <= 2 aggregate-first GCN layers; else falls back) */
    int32_t cone;          /* 0 = every layer is evaluated on every subgraph row, as DGL does (reference-equivalent
                              schedule, default); 1 = receptive-field schedule: only the centre rows of the last GCN layer
                              reach the head (learner.py:159-170), so layer l is evaluated only on the rows that are
                              (L-l) in-hops upstream of a centre, forward and backward -- the same sums for every row
                              that matters, nothing for the rows that cannot influence logits or gradients.
                              Supersedes sparse_bwd; falls back to the dense schedule if a pair has i == j */
    /* Batches of a WEIGHTED store (gm_store_create_weighted): every schedule CARRIES the weights, none falls back.  hoist_z1 needs nothing (the
       hoisted aggregate is the dense schedule's own launch); sparse_bwd reads a per-edge coefficient (weight x source norm) for the centres'
       in-edges beside their norms; cone copies the batch's per-edge weight / coefficient tables into its level CSRs.  With all weights 1.0
       each schedule returns its unweighted floats bit for bit.  gm_set_split_pieces(2) is ignored on weighted batches (three pieces,
       violation word 0): the two-piece magnitude bounds assume edge scales <= 1. */
} gm_hparams_t;

const char* gm_last_error(void);
int gm_version(void);

/* ---- GraphStore: replaces the list of DGLGraph objects + `feat` list (train.py:41-44,63-65).
 * indptr[g] (host int64[n_nodes[g]+1]) / indices[g] (host int32) = IN-edge CSR of graph g:
 * row v lists the sources u of every edge u->v (parallel edges and self loops kept, DGL
 * multigraph semantics of G.in_edges(v), sdp.py:301).  feat[g] = host fp32 [n_nodes[g], feat_dim]. */
int gm_store_create(int32_t n_graphs, const int64_t* n_nodes, const int64_t* const* indptr,
                    const int32_t* const* indices, const float* const* feat, int32_t feat_dim,
                    gm_store_t** out);
/* The same with a strength on every edge (beyond the reference): weights[g] (host fp32, aligned with indices[g]) = w_uv of the edge u->v,
 * finite and > 0 (GM_EINVAL otherwise; the message names the graph and the edge).  weights == NULL is gm_store_create.  Extraction stays
 * purely topological (hops, the sampling threshold and keys, the node order never look at a weight); a batch cut from a weighted store carries
 * the induced weights (GM_F_EDGE_W / GM_F_EDGE_W_T), and in fp32
 *   d(v) = sum of w_uv over the in-edges of v inside its subgraph, in the row's edge order;   GM_F_NORM(v) = 1 / sqrtf(d(v) > 0 ? d(v) : 1);
 *   GraphConv: relu(norm(v) * sum_{u->v} w_uv * norm(u) * x[u] W + b), both branch orders of learner.py:34-47; the backward uses the same
 *   coefficients on the by-source CSR; weights are constants (no gradient).
 * Integer weights equal the multigraph with the edge repeated w_uv times; all weights 1.0 give the unweighted floats bit for bit.
 * gm_store_weighted / gm_batch_weighted: 1 for a store created with weights / a batch cut from one. */
int gm_store_create_weighted(int32_t n_graphs, const int64_t* n_nodes, const int64_t* const* indptr,
                             const int32_t* const* indices, const float* const* weights, const float* const* feat, int32_t feat_dim,
                             gm_store_t** out);
int32_t gm_store_weighted(const gm_store_t* s);
void gm_store_destroy(gm_store_t* s);

/* ---- NEGATIVE PAIRS for link prediction, drawn on the device (beyond the reference, which draws them on the host and stores them as false
 * edges, data_process/link_process.py:83-85).  This comment is THE definition; tests/negative_ref.py restates it one candidate at a time and the
 * device result equals it bit for bit.  Per parent graph g of a store with N >= 2 nodes, seed (u64) and mode m:
 *   modes        GM_NEG_UNIFORM (0): both endpoints uniform over the nodes.  GM_NEG_TWO_HOP (1): a uniform, b two out-steps from a -- the hard
 *                negatives that share a neighbour.
 *   random words s = sample_salt(seed, g, 0x6E454721, m) (the salt of the extraction's keyed permutation: csrc/extract.hip, oracle.sample_salt);
 *                r(k, c) = lowbias32(s + 4 k + c) in 32-bit wrap-around arithmetic, k = 0, 1, 2, ..., c in 0..3;
 *                pick(r, n) = (uint64(r) * n) >> 32.
 *   candidate k  uniform:  a = pick(r(k,0), N), b = pick(r(k,1), N).
 *                two-hop, on the out-CSR rows with parallel copies kept (out[x] = destinations of x's out-edges, ascending):
 *                a = pick(r(k,0), N);  w = out[a][pick(r(k,1), outdeg(a))];  b = out[w][pick(r(k,2), outdeg(w))];
 *                the candidate is invalid if either out-degree is 0.
 *                Canonical form: (u, v) = (min(a, b), max(a, b)).
 *   valid        iff u != v, AND the graph holds no edge u -> v and no edge v -> u at any multiplicity (self loops elsewhere are irrelevant, edge
 *                weights are ignored), AND the key u * N + v (int64) is not in the caller's exclusion list: d_exclude_keys, n_exclude sorted
 *                unique int64 keys on the device (n_exclude = 0: none).
 *   result       the first n DISTINCT valid pairs in ascending order of k -- a pair counts where its smallest k is -- written to d_out_pairs
 *                (device int32 [n, 2], u < v) in that order.  The draw budget is 64 n + 4096 candidates: if it holds fewer than n distinct valid
 *                pairs the call still returns GM_OK, *h_found (host) is the count found and only that many rows of d_out_pairs are written;
 *                otherwise *h_found = n.
 * The result is a function of (graph, seed, mode, exclusion list, n) alone: it does not depend on how the candidate stream is cut into rounds
 * (gm_set_tuning("neg_round", R): candidates per round, 0 = the library's choice) nor on the stream.  The call runs on `stream`, takes its
 * scratch from the stream-ordered pool, and returns after the stream has produced the pairs (it reads one counter per round).
 * GM_EINVAL: a bad graph index, N < 2, n < 0, an unknown mode, or n above (2^31 - 1 - 4096) / 64 (the budget must fit int32 counters).
 * gm_store_has_edges: the sampler's adjacency test for n given pairs (device int32 [n, 2], any orientation): d_out[k] = 1 where the graph holds
 * an edge between the two nodes in either direction (for a pair (a, a): a self loop), else 0; 0 for a node id outside the graph. */
#define GM_NEG_UNIFORM 0
#define GM_NEG_TWO_HOP 1
int32_t gm_store_negative_pairs(const gm_store_t* s, int32_t g, int64_t n, uint64_t seed, int32_t mode, const int64_t* d_exclude_keys,
                                int64_t n_exclude, int32_t* d_out_pairs, int64_t* h_found, void* stream);
int32_t gm_store_has_edges(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, uint8_t* d_out, void* stream);

/* ---- HELD-OUT EDGES (beyond the reference): a store derived on the device from a resident one with a set of node pairs removed, and the deterministic
 * random split of a graph's links that produces such a set -- the evaluation protocol of link prediction, where the graph the structural inputs are
 * computed from holds none of the links being predicted.  This comment is THE definition; tests/holdout_ref.py restates it and the device result
 * equals it bit for bit.
 * gm_store_without_edges(s, d_keys, h_key_off, out, stream)
 *   input    per graph g of the store (N_g nodes) a sorted, strictly ascending list of canonical keys u * N_g + v (int64), u <= v -- the format of
 *            gm_store_negative_pairs' exclusion list; u == v names self loops.  The lists are concatenated over the graphs in d_keys (device);
 *            h_key_off (host, [n_graphs + 1], h_key_off[0] = 0) gives their offsets.  Any list may be empty (d_keys may be NULL when all are).
 *   effect   *out is a new, independent store (gm_store_destroy, in any order relative to s) with the nodes and features of s and every stored edge
 *            a -> b of s except those whose canonical pair (min(a, b), max(a, b)) is listed for its graph: both directions and every parallel copy
 *            go; keys that name no edge are ignored; edge weights travel with their edges.
 *   contract the new store equals, bit for bit, the store gm_store_create / gm_store_create_weighted builds from the FILTERED in-CSR -- the rows of s
 *            with the removed entries deleted and the stored order otherwise kept: both CSR orientations and their weights, the node and edge
 *            offsets, the symmetric flag (decided on the device from the new arrays; env GM_EXTRACT_NO_SYM and a store without edges give false,
 *            and a non-symmetric parent can become symmetric), the feature table, its stride, bound and host statistics (copied device to device).
 *            The neighbour index is not copied: the new store builds its own at first use.
 *   errors   GM_EINVAL for a NULL argument, offsets that are not monotone, a key outside [0, N_g^2) or a list that is not strictly ascending (checked
 *            on the device in the same pass).  The call runs on `stream`, takes scratch from the stream-ordered pool and returns when the new
 *            store is complete.
 * gm_store_split_edges(s, g, seed, t_test, t_val, d_out_pairs, d_out_class, capacity, h_counts, stream): a Bernoulli split of the links of graph g,
 * decided per pair by a hash: a function of (graph, seed, thresholds) alone.
 *   links    the pairs (u, v), u < v, with v in the neighbour-index row of u (the distinct neighbours in either direction, as gm_store_pair_scores
 *            defines them): distinct, self loops never count.
 *   hash     s0 = sample_salt(seed, g, 0x53504C54, 0);  h(u, v) = lowbias32(lowbias32(s0 + (uint32)u) + (uint32)v) in 32-bit wrap-around arithmetic.
 *   class    2 (test) if h < t_test; 1 (validation) if t_test <= h < t_val; 0 (train) otherwise.  0 <= t_test <= t_val <= 2^32 (GM_EINVAL otherwise); a
 *            caller forms the thresholds as floor(fraction * 2^32) in integers.
 *   output   h_counts (host, [3]) = {links, validation, test}.  With d_out_pairs == NULL only the counts are produced; otherwise the held-out pairs
 *            (class 1 or 2) are written in ascending order of u * N + v to d_out_pairs (device int32 [n, 2]) and their classes to d_out_class (device
 *            uint8 [n]; may be NULL).  GM_ERANGE if `capacity` (rows of d_out_pairs) is below the held-out count.
 * gm_store_dims: nodes and stored edges of graph g, and the store's symmetric flag (any of the three may be NULL).  gm_store_read_csr: the CSR of graph
 * g as the store holds it, orientation 0 = by destination (entries = sources), 1 = by source (entries = destinations): h_ptr (host int64 [N + 1],
 * graph-local offsets), h_idx (host int32 [edges], graph-local ids), h_w (host fp32 [edges], weighted stores only; may be NULL).  Plain read-backs. */
int32_t gm_store_without_edges(const gm_store_t* s, const int64_t* d_keys, const int64_t* h_key_off /* host [n_graphs + 1] */, gm_store_t** out, void* stream);
int32_t gm_store_split_edges(const gm_store_t* s, int32_t g, uint64_t seed, uint64_t t_test, uint64_t t_val, int32_t* d_out_pairs, uint8_t* d_out_class,
                             int64_t capacity, int64_t* h_counts /* host [3] */, void* stream);
int32_t gm_store_dims(const gm_store_t* s, int32_t g, int64_t* n_nodes, int64_t* n_edges, int32_t* symmetric);
int32_t gm_store_read_csr(const gm_store_t* s, int32_t g, int32_t orientation, int64_t* h_ptr, int32_t* h_idx, float* h_w);

/* ---- NEIGHBOURHOOD HEURISTIC SCORES of node pairs (beyond the reference): the numbers a learned link predictor is held against -- common neighbours,
 * Jaccard, Adamic-Adar, resource allocation, preferential attachment -- for n pairs of one parent graph, on the device.  This comment is THE definition;
 * tests/pair_score_ref.py restates it with Python sets and fp64 sums.  Per parent graph g of a store, with N nodes:
 *   neighbourhood  G(x) = { z != x : the graph holds an edge x -> z or z -> x }: DISTINCT nodes -- parallel copies count once, self loops never count,
 *                  edge weights are ignored.  deg(x) = |G(x)|.
 *   node terms     w_aa(z) = 1 / ln(deg z) for deg z >= 2, else 0;  w_ra(z) = 1 / deg z for deg z >= 1, else 0: computed in double, rounded once to fp32.
 *   pairs          d_pairs: device int32 [n, 2].  A pair (a, b) may come in any orientation and a == b is allowed; it is canonicalised to (min, max)
 *                  first, so the result is bitwise the same for (a, b) and (b, a).
 *   mask flag      GM_PAIR_MASK_TARGET (1) in `flags` scores the pair as if no edge joined a and b (it mirrors GM_LINK_MASK_TARGET): with the flag, when
 *                  a != b and b in G(a), da = deg a - 1 and db = deg b - 1; otherwise -- and always without the flag -- da = deg a, db = deg b.
 *   five scores    I = G(a) & G(b) (it never holds a or b when a != b; for a == b it is G(a)).  d_out: device fp32 [n, 5], columns
 *                    0  cn                  = |I|
 *                    1  jaccard             = |I| / U, 0 when U == 0;  a != b: U = da + db - |I|;  a == b: U = deg a
 *                    2  adamic_adar         = sum of w_aa(z) over z in I
 *                    3  resource_allocation = sum of w_ra(z) over z in I
 *                    4  pref_attachment     = (float)((int64)da * db)
 *   out of range   a node id outside the graph gives five zeros, as gm_store_has_edges gives 0.
 *   exactness      cn and pref_attachment are exact (the integer, rounded once to fp32).  Columns 1-3 are fp32 quotients / sums; the order of a sum belongs
 *                  to the launch configuration (lanes per pair: the library picks it per launch from the graph's mean distinct degree;
 *                  gm_set_tuning("pair_lanes", L) with L in {16, 32, 64} forces one, 0 restores the library's choice).  For one configuration two runs
 *                  are bitwise identical: no float atomics, nothing depends on arrival order.
 * The scores read a neighbour index of the store -- per node the ascending distinct G row, deg, w_aa, w_ra; at most 2 |E| ints + 20 bytes per node --
 * built once per store by the first call that needs it (on the host, under a lock, and complete on the device before that call goes on: later calls read
 * it from any stream) and freed by gm_store_destroy.  Both calls run on `stream`; n == 0 is a no-op.
 * gm_store_neighbour_degrees: deg(x) of every node of graph g, device int32 [N].
 * GM_EINVAL: a bad graph index, n < 0, unknown flag bits, a pair_lanes value that is no instantiation. */
#define GM_PAIR_MASK_TARGET 1
int32_t gm_store_pair_scores(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, float* d_out, void* stream);
int32_t gm_store_neighbour_degrees(const gm_store_t* s, int32_t g, int32_t* d_out, void* stream);

/* ---- CANDIDATE PARTNERS for link prediction (beyond the reference): which pairs to score at all.  For m source nodes of one parent graph, the non-adjacent
 * nodes that share a neighbour with the source, ranked by one pair score, the best k of each -- on the device.  This comment is THE definition;
 * tests/candidate_ref.py restates it with Python sets.  Per parent graph g of a store with N nodes:
 *   neighbourhood  G(x) and deg are those of gm_store_pair_scores: DISTINCT nodes in either direction, self loops never count, weights are ignored.
 *   candidate set  C(a) = { w : w != a, w not in G(a), G(a) & G(w) not empty }: the nodes at distance exactly 2 in the distinct-neighbour graph.
 *                  d_nodes: device int32 [m] sources.  Duplicate sources are allowed, every row of the result is independent.  A source id outside [0, N)
 *                  has C = {} (as gm_store_pair_scores gives five zeros for a node outside the graph).
 *   score          column `col` (0..4, the order of gm_store_pair_scores: cn, jaccard, adamic_adar, resource_allocation, pref_attachment) of
 *                  gm_store_pair_scores for the pair (a, w) with flags 0 (a candidate is never adjacent: the mask flag would change nothing), BITWISE equal to
 *                  it under the lanes-per-pair configuration in force (the library's choice or gm_set_tuning("pair_lanes")).  Every candidate has cn >= 1
 *                  and both degrees >= 1, so every score is a positive finite fp32.
 *   ranking        descending score, among equal fp32 scores ascending node id w: the descending order of the integer key
 *                  (uint64(score bits) << 32) | (0xFFFFFFFF - w).  Selection is integer work and the result is unique.
 *   result         for k in 1..1024: d_out_nodes device int32 [m, k], d_out_scores device fp32 [m, k], d_out_total device int32 [m] = |C(a)|.  Row r holds
 *                  the first min(k, total[r]) candidates of the ranking, in ranking order; the remaining entries are -1 in d_out_nodes and 0.0f in
 *                  d_out_scores.  Nothing beyond row m - 1 is written.
 * The result is a function of (graph, sources, k, col, lanes-per-pair configuration) alone: not of the stream, not of how the sources are cut into rounds
 * (gm_set_tuning("cand_round", P): pairs per round, 0 = the library's choice; a source whose set alone exceeds P gets a round of its own), not of where the
 * membership bitmap of the enumeration lives (gm_set_tuning("cand_bitmap", 0 | 1 | 2): the library's choice, LDS, a slab in HBM; forcing LDS on a graph
 * of more than 262,144 nodes is GM_EINVAL).  Two runs agree bit for bit: no float atomics, nothing depends on arrival order.
 * The call reads the neighbour index (built at first use, as for gm_store_pair_scores), runs on `stream`, takes its scratch from the stream-ordered pool,
 * reads the set sizes back once to cut the rounds, and returns after the stream has produced the result.  m == 0 is a no-op.
 * GM_EINVAL (the message names the value): a bad graph index, m < 0 or above INT32_MAX, k outside 1..1024, col outside 0..4, a NULL argument with m > 0,
 * a pair_lanes value that is no instantiation, a bad cand_bitmap / cand_round.  GM_ERANGE: a round whose pair count passes 2^31 - 1. */
int32_t gm_store_pair_candidates(const gm_store_t* s, int32_t g, const int32_t* d_nodes, int64_t m, int32_t k, int32_t col, int32_t* d_out_nodes,
                                 float* d_out_scores, int32_t* d_out_total, void* stream);

/* ---- WALK COUNTS of node pairs (beyond the reference): the numbers of walks of length 1, 2 and 3 between the two nodes of n pairs of one parent graph, on the
 * device -- what the heuristics one step beyond the common neighbours are made of: the local path index w2 + eps w3 and the truncated Katz index
 * beta w1 + beta^2 w2 + beta^3 w3 (formed on the host from these integers: g-meta_amd/heuristics.py).  This comment is THE definition;
 * tests/path_walk_ref.py restates it with Python sets.  Per parent graph g of a store, with N nodes:
 *   neighbourhood  G(x) and deg are those of gm_store_pair_scores: DISTINCT nodes joined in either direction, self loops never count, parallel copies count
 *                  once, weights are ignored.  S is the symmetric 0 / 1 matrix of G.
 *   pairs          d_pairs: device int32 [n, 2].  Any orientation and a == b are allowed; a pair is canonicalised to (u, v) = (min, max) first, so (a, b) and
 *                  (b, a) give the same row.
 *   result         d_out: device int64 [n, 3], columns
 *                    0  w1 = (S)[u, v]   = [v in G(u)]
 *                    1  w2 = (S^2)[u, v] = sum over z in G(u) of [z in G(v)]: cn for u != v, deg u for u == v
 *                    2  w3 = (S^3)[u, v] = sum over z in G(u) of |G(z) & G(v)|
 *                  S^3 is symmetric: the value does not depend on which endpoint is expanded.
 *   mask flag      GM_PAIR_MASK_TARGET (1) in `flags` counts the walks in S without the edge {u, v}: when u != v and v in G(u), w1 = 0, w2 is unchanged and w3
 *                  loses deg u + deg v - 1 (deg v walks whose first step is u -> v, deg u whose last step is, u v u v in both; the middle step cannot be the
 *                  edge alone).  Otherwise -- and always without the flag -- nothing changes.
 *   out of range   a node id outside [0, N) gives three zeros.
 *   exactness      integer work throughout; w3 <= deg u * deg v < 2^62.  The result is a function of (graph, pairs, flags) alone: the lanes per work item
 *                  (gm_set_tuning("walk_lanes", L) with L in {32, 64} -- the widths that are built -- forces one, 0 restores the library's choice by the
 *                  graph's mean distinct degree and the length of the pair list), the way a pair's work is cut (gm_set_tuning("walk_chunk", C): entries of the expanded endpoint's row per
 *                  work item, 0 = the library's choice; a pair whose row is longer is summed by several items with 64-bit integer atomic adds onto its
 *                  seeded row), the stream and the arrival order cannot change a bit of it.
 *   writes         the rows of all n pairs, duplicates included (every row is seeded and summed on its own); nothing behind row n - 1.
 * The call reads the neighbour index (built at first use, as for gm_store_pair_scores), runs on `stream`, takes its scratch from the stream-ordered pool and
 * reads two counters back once to size the launch over the heavy pairs' items; the result is complete in stream order.  n == 0 is a no-op.
 * GM_EINVAL (the message names the value): a bad graph index, n < 0 or above INT32_MAX, unknown flag bits, a NULL argument with n > 0, a negative walk_chunk,
 * a walk_lanes value that is no instantiation.  GM_ERANGE: more than 2^30 work items in one call (a walk_chunk far too small for the pairs). */
int32_t gm_store_pair_walks(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, int64_t* d_out, void* stream);

/* ---- ROOTED PAGERANK of sources and node pairs (beyond the reference): the one GLOBAL score among the baselines a link predictor is held against -- the
 * stationary mass a walk from s that returns to s with probability alpha leaves on every node, after a fixed number of steps, on the device.  This comment is
 * THE definition; tests/pagerank_ref.py restates it in float64.  Per parent graph g of a store, with N nodes:
 *   neighbourhood  G(x) and deg are those of gm_store_pair_scores: DISTINCT nodes joined in either direction, self loops never count, parallel copies count
 *                  once, weights are ignored.
 *   column         a pair (s, x): s the source, x = -1 or a node whose edge {s, x} is removed.  The column's graph G' is G when x = -1, x == s or x not in
 *                  G(s); otherwise G without that one edge: only the rows of s and x lose an entry, deg' s = deg s - 1, deg' x = deg x - 1.
 *   walk           a = (float)alpha, b = 1.0f - a, in fp32.  p_0 = e_s; for t = 0 .. iters - 1:  p_{t+1}[v] = a [v == s] + b m_t[v], where
 *                  m_t[v] = sum over z in G'(v) of p_t[z] / deg' z when deg' v > 0, and m_t[v] = p_t[v] when deg' v == 0: a node without neighbours keeps
 *                  its mass.  So the walk keeps its mass -- sum_v p_{t+1}[v] = a + b sum_v p_t[v]: 1 up to the rounding of b and of the sums -- and an isolated source
 *                  gives p = e_s for every t (in fp32 a + b rounds to 1.0f).  pi_(s,x) = p_iters, fp32.
 *                  0 < alpha < 1, finite; iters in 1 .. 255.
 *   gm_store_rooted_pagerank   d_sources: device int32 [m]; d_out: device fp32 [m, N], row r = pi_(sources[r], -1).  Duplicates are allowed, every row is
 *                  written on its own; a source outside [0, N) gives a row of zeros.  Nothing behind row m - 1 is written.
 *   gm_store_pair_pagerank     d_pairs: device int32 [n, 2], any orientation, a == b allowed; a pair is canonicalised to (u, v) = (min, max).  d_out: device
 *                  fp32 [n, 2].  Without a flag column 0 = pi_(u,-1)[v], column 1 = pi_(v,-1)[u].  With GM_PAIR_MASK_TARGET (1) in `flags` column 0 =
 *                  pi_(u,v)[v], column 1 = pi_(v,u)[u]: the score in the graph without the pair's own edge, as the other two pair calls mask it; a
 *                  non-adjacent pair gives the bits of the unflagged call.  A node outside the graph gives two zeros.  The score pi_u(v) + pi_v(u) is formed
 *                  on the host in float64 (g-meta_amd/heuristics.py), as the path scores are.
 *   exactness      no float atomics, nothing depends on arrival order.  A row sum runs in ascending neighbour order; a row of more than C entries is summed
 *                  in segments of C whose partial sums are added in ascending order (gm_set_tuning("ppr_chunk", C), 0 = the library's choice): the order of
 *                  a row sum belongs to that configuration, as the order of a score sum belongs to pair_lanes.  For one value of ppr_chunk a row of either
 *                  result is bit for bit a function of (graph, its own source or pair, flags, alpha, iters) alone: not of the other rows of the call, their
 *                  order or their duplicates, not of how many columns a round holds (gm_set_tuning("ppr_cols", B), a multiple of 64 up to 4096, 0 = the
 *                  library's choice), not of the stream; and the same from either export: gm_store_pair_pagerank without the flag gives the entries of
 *                  gm_store_rooted_pagerank's rows, bitwise.
 * Both calls read the neighbour index (built at first use, as for gm_store_pair_scores), run on `stream`, take their scratch -- two fp32 [N, B] states and
 * the hub rows' partial sums -- from the stream-ordered pool, and read the sources or pairs (and the graph's row lengths) back once to form the distinct
 * columns; the result is complete in stream order.  n == 0 / m == 0 is a no-op.
 * GM_EINVAL (the message names the value): a bad graph index, n / m negative or above INT32_MAX, unknown flag bits, alpha outside (0, 1) or not finite, iters
 * outside 1 .. 255, a NULL argument with work to do, a negative ppr_chunk, a ppr_cols that is no multiple of 64 or above 4096. */
int32_t gm_store_rooted_pagerank(const gm_store_t* s, int32_t g, const int32_t* d_sources, int64_t m, float alpha, int32_t iters, float* d_out, void* stream);
int32_t gm_store_pair_pagerank(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, float alpha, int32_t iters, float* d_out,
                               void* stream);

/* ---- CANDIDATE PARTNERS BY ROOTED PAGERANK (beyond the reference): for m source nodes of one parent graph the k non-adjacent nodes that hold the most
 * rooted-PageRank mass seen from the source -- the global generator beside gm_store_pair_candidates, selected on the device from the walk's state while it is
 * still in scratch: only [m, k] leaves it.  This comment is THE definition; tests/pagerank_candidate_ref.py restates it.  Per parent graph g with N nodes:
 *   neighbourhood  G(x), deg and the walk are those of gm_store_rooted_pagerank.
 *   score          of w for the source a: pi_(a,-1)[w], the entry of gm_store_rooted_pagerank's row for a, BITWISE, under the ppr_chunk in force.  The score is
 *                  one-directional; the symmetric pi_a(w) + pi_w(a) would need a column per candidate: a caller who wants it rescores the shortlist with
 *                  gm_store_pair_pagerank.
 *   candidate set  R(a) = { w : w != a, w not in G(a), pi_(a,-1)[w] > 0 }, decided on the fp32 bits: an entry that underflowed to zero is no candidate.
 *                  Unlike C(a) of gm_store_pair_candidates, R(a) reaches every node within `iters` steps of a.  An isolated source and a source outside
 *                  [0, N) have R = {}.
 *   ranking        descending score, among equal fp32 scores ascending node id w: the descending order of the integer key
 *                  (uint64(score bits) << 32) | (0xFFFFFFFF - w), the key of gm_store_pair_candidates.  Selection is integer work and the result is unique.
 *   result         for k in 1..1024: d_out_nodes device int32 [m, k], d_out_scores device fp32 [m, k], d_out_total device int32 [m] = |R(a)|.  Row r holds
 *                  the first min(k, total[r]) candidates of the ranking, in ranking order, then -1 in d_out_nodes and 0.0f in d_out_scores.  Nothing beyond
 *                  row m - 1 is written.  Duplicate sources are allowed and give identical rows.
 *   exactness      a row is a function of (graph, its own source, k, alpha, iters, ppr_chunk) alone: not of the other rows, of ppr_cols, of the stream or
 *                  of arrival order.  No float atomics; integer atomics only where their order cannot change the result (histogram counts, list slots
 *                  ahead of a sort of unique keys).
 * The call reads the neighbour index, runs on `stream`, takes its scratch -- the walk's, a 256-bin histogram and at most 1,024 keys per column of a round --
 * from the stream-ordered pool, reads the sources (and the graph's row lengths) back once, and is complete in stream order.  m == 0 is a no-op.
 * GM_EINVAL (the message names the value): as gm_store_rooted_pagerank, and k outside 1..1024. */
int32_t gm_store_pagerank_candidates(const gm_store_t* s, int32_t g, const int32_t* d_nodes, int64_t m, int32_t k, float alpha, int32_t iters,
                                     int32_t* d_out_nodes, float* d_out_scores, int32_t* d_out_total, void* stream);

/* ---- SHORTEST-PATH DISTANCES of sources and node pairs (beyond the reference): graph distance, the first of the classical link-prediction baselines, and the
 * answer to "which nodes lie within d hops" and "is this edge a bridge, and if not how long is the detour" -- a bit-parallel breadth-first search of many
 * columns at once, on the device.  This comment is THE definition; tests/distance_ref.py restates it with a plain breadth-first search.  Per parent graph g of
 * a store, with N nodes:
 *   neighbourhood  G(x) is that of gm_store_pair_scores: DISTINCT nodes joined in either direction, self loops never count, parallel copies count once,
 *                  weights are ignored.
 *   column         a pair (s, x), exactly as for gm_store_rooted_pagerank: s the source, x = -1 or a node whose edge {s, x} is removed.  The column's graph G'
 *                  is G when x = -1, x == s or x not in G(s); otherwise G without that one edge.
 *   distance       d_(s,x)[v] = the number of edges on a shortest path from s to v in G'; 0 for v == s; UNREACHED when there is no path or the shortest one
 *                  is longer than max_dist.  max_dist in 1 .. 254; unreached is the byte 255 (GM_DIST_UNREACHED) in both results.
 *   gm_store_node_distances   d_sources: device int32 [m]; d_out: device uint8 [m, N], row r = d_(sources[r], -1).  Duplicates are allowed, every row is
 *                  written on its own; a source outside [0, N) gives a row of 255.  Nothing behind row m - 1 is written.
 *   gm_store_pair_distance    d_pairs: device int32 [n, 2], any orientation, a == b allowed; a pair is canonicalised to (u, v) = (min, max).  d_out: device
 *                  uint8 [n].  Without a flag the entry is d_(u,-1)[v].  With GM_PAIR_MASK_TARGET (1) in `flags` it is d_(u,v)[v]: the distance in the graph
 *                  without the pair's own edge, as the other pair calls mask it (G' is symmetric, so d_(v,u)[u] is the same number: one column per pair);
 *                  a non-adjacent pair gives the unflagged byte.  a == b gives 0; a node outside the graph gives 255.
 *   exactness      the results are integers and unique.  A row or entry is a function of (graph, its own source or pair, flags, max_dist) alone: not of the
 *                  other rows of the call, their order or their duplicates, not of how many columns a round holds (gm_set_tuning("dist_cols", B), a multiple
 *                  of 64 up to 4096, 0 = the library's choice), not of where a long row is cut (gm_set_tuning("dist_chunk", C): entries per segment of a
 *                  row of more than C, C >= 0, 0 = the library's choice), not of the stream or of arrival order.  gm_store_pair_distance without the flag
 *                  gives the entries of gm_store_node_distances' rows.
 * Both calls read the neighbour index (built at first use, as for gm_store_pair_scores), run on `stream`, take their scratch -- three bit matrices of
 * N x B / 8 bytes each, B = the columns of a round, and 8 bytes per hub segment and 64 columns -- from the stream-ordered pool, and read the sources or pairs
 * (and the graph's row lengths) back once to form the distinct columns; a call with max_dist above 16 also reads one flag back every 16 levels to stop early.
 * The result is complete in stream order.  n == 0 / m == 0 is a no-op.
 * GM_EINVAL (the message names the value): a bad graph index, n / m negative or above INT32_MAX, unknown flag bits, max_dist outside 1 .. 254, a NULL argument
 * with work to do, a negative dist_chunk, a dist_cols that is no multiple of 64 or above 4096. */
#define GM_DIST_UNREACHED 255
int32_t gm_store_node_distances(const gm_store_t* s, int32_t g, const int32_t* d_sources, int64_t m, int32_t max_dist, uint8_t* d_out, void* stream);
int32_t gm_store_pair_distance(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, int32_t max_dist, uint8_t* d_out, void* stream);

/* ---- JOINT HOP-DISTANCE PROFILES of node pairs (beyond the reference): for a pair (u, v) the number of nodes lying a hops from u and b hops from v, for all
 * small a, b -- the table behind SEAL's double-radius labels and the structure features of ELPH / BUDDY, exact, counted on the device from the state of the
 * search above so that only [n, D + 2, D + 2] integers leave it.  This comment is THE definition; tests/distance_profile_ref.py restates it.  Per parent graph g
 * of a store, with N nodes:
 *   columns        neighbourhoods, columns (s, x) and d_(s,x)[z] are exactly those of gm_store_node_distances / gm_store_pair_distance.
 *   D, cap         D = max_dist, in 1 .. 7 (the range of gm_set_hop_labels; a table has (D + 2)^2 <= 81 entries).  cap(d) = d if d <= D, else D + 1: the farther
 *                  nodes and the unreached ones (byte 255) alike.
 *   pair           d_pairs: device int32 [n, 2], any orientation, p == q allowed; a pair is canonicalised to (u, v) = (min, max).  xu = v and xv = u when
 *                  GM_PAIR_MASK_TARGET (1) is in `flags`, u != v and v in G(u); otherwise xu = xv = -1.
 *   table          P[a][b] = |{ z in [0, N) : cap(d_(u,xu)[z]) == a and cap(d_(v,xv)[z]) == b }|,   a, b in 0 .. D + 1
 *   result         d_out: device int32 [n, D + 2, D + 2], row-major [a][b] of the CANONICAL pair: both orientations of a pair give the same bits (the table of
 *                  (v, u) is the transpose; g-meta_amd/heuristics.py orients it by the pair's name).  A pair with a node outside the graph gives all zeros.
 *                  Nothing behind entry n - 1 is written.  Duplicates are allowed, every entry is written on its own.
 *   identities     that follow from the definition (tests hold the device to them):
 *                    sum of P = N;
 *                    row 0 and column 0 hold a single 1 each, at cap(gm_store_pair_distance(pair, flags)); u == v: P[0][0] = 1 and P is diagonal;
 *                    u != v: P[1][1] = cn of gm_store_pair_scores, flagged or not (the pair's own edge never joins a common neighbour);
 *                    sum over b of P[a][b] = |{ z : cap(d_(u,xu)[z]) == a }|, and the column sums likewise for v;
 *                    a non-adjacent pair under the flag gives the unflagged bits.
 *   exactness      the results are integers and unique.  A table is a function of (graph, its own pair, flags, max_dist) alone: not of the other pairs of the
 *                  call, their order or their duplicates, not of dist_cols or dist_chunk (above), not of gm_set_tuning("dist_plane_kib", K) (below), not of
 *                  the stream.  No atomics.
 * The call reads the neighbour index, runs on `stream`, reads the pairs (with the flag their adjacency bytes, and the graph's row lengths) back once, sorts the
 * canonical pairs by (u, v) and cuts them into groups of at most Bp DISTINCT columns, so that both columns of a pair are alive in one round of the search; each
 * group is searched on its own.  Scratch from the stream-ordered pool: the search's (above, B = the widest group's columns), the level planes -- one bit per
 * (level 0 .. D, column, node): (D + 1) x Bp x ceil(N / 64) x 8 bytes -- and 16 bytes per pair.  Bp = min(dist_cols in force, the largest multiple of 64 whose
 * planes fit the budget); the budget is gm_set_tuning("dist_plane_kib", K) / GM_DIST_PLANE_KIB in KiB, 0 = the library's choice, 1 GiB.  GM_ERANGE (the message
 * names N, max_dist and the budget) when the planes of even 64 columns do not fit.  The result is complete in stream order.  n == 0 is a no-op, with NULL
 * pointers too.
 * GM_EINVAL (the message names the value): as gm_store_pair_distance, with max_dist outside 1 .. 7, and a negative dist_plane_kib. */
int32_t gm_store_pair_distance_profile(const gm_store_t* s, int32_t g, const int32_t* d_pairs, int64_t n, int32_t flags, int32_t max_dist, int32_t* d_out, void* stream);

/* ---- NEIGHBOURHOOD SKETCHES of all nodes (beyond the reference): the ELPH / BUDDY route to the table above for EVERY training pair.  The exact profile costs a
 * search of two columns per pair; here each node carries a HyperLogLog and a MinHash sketch of its d-hop ball for d = 0 .. H, built once by H rounds of
 * element-wise max / min over the neighbour lists, and the joint table of any pair is estimated from 2 (H + 1) small records with no search.  This comment is
 * THE definition; tests/sketch_ref.py restates it.  Per parent graph g of a store, with N nodes:
 *   neighbourhood  G(x) is that of gm_store_pair_scores: DISTINCT nodes joined in either direction, self loops never count, parallel copies count once,
 *                  weights are ignored.
 *   parameters     hops H in 1 .. 4; HLL precision p in 4 .. 10, m = 2^p registers of one byte; MinHash width K, a multiple of 32 in 32 .. 512, uint32
 *                  values; seed, u64.
 *   hashes         lowbias32 and sample_salt are those of the node sampling (gm_extract).  s_h = sample_salt(seed, g, 0x534B4831, 0),
 *                  s_m = sample_salt(seed, g, 0x534B4D31, 0).
 *                  HLL insert of node z:  h = lowbias32((uint32) z ^ s_h); register j = h >> (32 - p); w = h << p (mod 2^32); rho = clz32(w) + 1 when
 *                  w != 0, else 33 - p.
 *                  MinHash of node z:  q = lowbias32((uint32) z ^ s_m); mh_k(z) = lowbias32(q + (k + 1) * 0x9E3779B9) in wrap-around arithmetic, k = 0 .. K - 1.
 *                  Every step is a bijection of uint32, so for a fixed k distinct nodes never share a value of mh_k: two of the identities below rest on it.
 *   balls          B_0(x) = {x};  B_d(x) = B_{d-1}(x) united with B_{d-1}(z) over z in G(x)  =  { z : gm_store_node_distances(x)[z] <= d }.
 *   sketches       R_d(x)[j] = max rho(z) over the z in B_d(x) with register j(z) = j, 0 if there is none;  M_d(x)[k] = min over z in B_d(x) of mh_k(z).
 *                  Both are functions of a set and therefore unique; the recurrence computes them as the element-wise max / min over x's own level d - 1
 *                  record and those of G(x).
 *   pair counts    d_pairs: device int32 [n, 2], any orientation, a == b allowed; a pair is canonicalised to (u, v) = (min, max).  For a, b in 0 .. H, with
 *                  U = max(R_a(u), R_b(v)) element-wise:
 *                    match[a][b] = |{ k : M_a(u)[k] == M_b(v)[k] }|
 *                    zeros[a][b] = |{ j : U[j] == 0 }|
 *                    zsum[a][b]  = sum over j of 2^(32 - U[j]), exact; below 2^43
 *                  d_out: device int64 [n, H + 1, H + 1, 3] = (match, zeros, zsum);  d_out_balls: device int64 [n, 2, H + 1, 2] = (zeros, zsum) of R_a(u) and
 *                  then of R_a(v) alone.  A node id outside [0, N) gives zeros in both.  Nothing behind entry n - 1 is written.  Duplicates are written
 *                  each on their own.  The estimators (HyperLogLog cardinality, MinHash Jaccard, the table in the layout of gm_store_pair_distance_profile)
 *                  over these integers are written twice: in float64 on the host (g-meta_amd/heuristics.py), and on the device in gm_sketch_pair_features.
 *   pair features  gm_sketch_pair_features: the S = (H + 2)^2 structure columns a BUDDY predictor reads, formed from the integers above without leaving the
 *                  device.  d_pairs as above; d_out: device float32 with row stride ld >= S; row e, columns 0 .. S - 1 get the features of pair e and NOTHING
 *                  else is written: not the columns S .. ld - 1, not anything behind row n - 1.  The chain below is evaluated in fp64 (IEEE double), each
 *                  operation as written and rounded once -- no fused multiply-add -- and tests/sketch_feature_ref.py restates it:
 *                    integers  (match, zeros, zsum)[a][b] and the ball entries of the canonical (u, v) = (min, max), exactly as pair counts gives them; a
 *                              node id outside [0, N) gives the chain's value on all-zero integers.
 *                    card(zeros, zsum), with m = 2^p:  s = zsum / 2^32;  est = ((alpha * m) * m) / s, or 0 where zsum == 0;  where zsum != 0 and
 *                              est <= 2.5 * m and zeros > 0 the value is m * log(m / zeros), else est.  alpha = 0.673, 0.697, 0.709 at m = 16, 32, 64, else
 *                              0.7213 / (1.0 + 1.079 / m).  (gmeta_amd.hll_cardinality, in its operation order.)
 *                    C[a][b] = (match[a][b] / K) * card(zeros[a][b], zsum[a][b]);  su[a] = card(u's ball entry a), sv[b] = card(v's ball entry b).
 *                    P, (H + 2) x (H + 2), with C[-1][.] = C[.][-1] = 0, su[-1] = sv[-1] = 0 (gmeta_amd.sketch_distance_profile):
 *                              P[a][b] = (C[a][b] - C[a-1][b]) - (C[a][b-1] - C[a-1][b-1])                      a, b in 0 .. H
 *                              P[a][H+1] = (su[a] - su[a-1]) - sum over b = 0 .. H of P[a][b]
 *                              P[H+1][b] = (sv[b] - sv[b-1]) - sum over a = 0 .. H of P[a][b]
 *                              P[H+1][H+1] = N - sum of all other cells
 *                              every sum runs from 0.0 over its cells in ascending index order (the last one row-major), one addition per cell.
 *                    T         symmetric != 0: T[a][b] = P[a][b] + P[b][a].  symmetric == 0: T = P for d_pairs[e] = (x, y) with x <= y, its transpose
 *                              otherwise -- entry [a][b] then speaks of the nodes a hops from x and b hops from y (gmeta_amd.link_sketch_profiles).
 *                    out[e][a * (H + 2) + b] = (float) log1p(max(T[a][b], 0)).
 *                  fp64 keeps the cancellation of the differences far below fp32 resolution and is the host definition's format; log and log1p are the
 *                  device library's (a few ulp), so the host chain agrees to fp32 rounding, not in every bit.  A pair's row is the same bits alone or in any
 *                  batch, on any stream, and for both orientations when symmetric.  No atomics.
 *   identities     that follow from the definition (tests hold the device to them): match[a][b] == K whenever B_a(u) == B_b(v); match[a][b] == 0 whenever the
 *                  two balls are disjoint (mh_k is a bijection); B_a(u) inside B_b(v) makes (zeros, zsum)[a][b] v's ball entry b; zeros and zsum do not
 *                  increase in a or in b; both orientations of a pair give the same bits.
 *   no mask flag   the sketches describe the WHOLE graph: a pair's own edge cannot be taken out of them (ELPH has the same limit).  The exact, masked table of
 *                  a shortlist is gm_store_pair_distance_profile with GM_PAIR_MASK_TARGET.
 *   exactness      every output is an integer and a function of (graph, seed, H, p, K, and for the counts the pair) alone: not of where a long row is cut
 *                  (gm_set_tuning("sketch_chunk", C): entries per segment of a row of more than C, 0 = the library's choice -- max and min are idempotent
 *                  and commutative), not of the stream, of arrival order or of the other pairs of the call.  No atomics, no floats.
 *   memory         a sketch owns N (H + 1) (2^p + 4 K) bytes of device memory (0.52 GB at N = 169,343, H = 3, p = 8, K = 128), laid out level-major, then
 *                  node-major, a node's record = its 2^p register bytes then its K words; level 0 is STORED, not recomputed.  gm_set_tuning("sketch_mib", M) /
 *                  GM_SKETCH_MIB is the budget of one build in MiB, 0 = the library's choice, 8 GiB: GM_ERANGE (the message names N, H, p, K and the budget)
 *                  when the formula exceeds it.  The sketch does not reference the store afterwards: destroying the store first is legal.
 * gm_store_sketch_build reads the neighbour index (built at first use, as for gm_store_pair_scores), runs on `stream`, reads the graph's row lengths back once
 * to cut the hub rows, takes the hub segments' partial records from the stream-ordered pool, and returns after the stream has produced the sketch: any stream
 * may read it afterwards.  gm_sketch_registers returns the raw records of m nodes at one level, d_hll: device uint8 [m, 2^p], d_minhash: device uint32 [m, K]; a
 * node outside [0, N) gives zeros.  Both readers run on `stream` and are complete in stream order; n == 0 / m == 0 is a no-op, with NULL pointers too.
 * gm_sketch_dims fills whichever of its outputs is not NULL (bytes: the formula above).  gm_sketch_destroy waits for the device and frees the records.
 * GM_EINVAL (the message names the value): a bad graph index, hops / p / k outside the ranges above, a level outside 0 .. H, n or m negative or above
 * INT32_MAX, a NULL argument with work to do, a negative sketch_chunk or sketch_mib, ld < (H + 2)^2. */
typedef struct gm_sketch gm_sketch_t;
int32_t gm_store_sketch_build(const gm_store_t* s, int32_t g, int32_t hops, int32_t p, int32_t k, uint64_t seed, void* stream, gm_sketch_t** out);
int32_t gm_sketch_dims(const gm_sketch_t* sk, int64_t* n_nodes, int32_t* hops, int32_t* p, int32_t* k, int64_t* bytes);
int32_t gm_sketch_registers(const gm_sketch_t* sk, int32_t level, const int32_t* d_nodes, int64_t m, uint8_t* d_hll, uint32_t* d_minhash, void* stream);
int32_t gm_sketch_pair_counts(const gm_sketch_t* sk, const int32_t* d_pairs, int64_t n, int64_t* d_out, int64_t* d_out_balls, void* stream);
int32_t gm_sketch_pair_features(const gm_sketch_t* sk, const int32_t* d_pairs, int64_t n, int32_t symmetric, float* d_out, int64_t ld, void* stream);
void gm_sketch_destroy(gm_sketch_t* sk);

/* ---- HOP-PROPAGATED NODE FEATURES of a whole parent graph (beyond the reference): the second precomputed input of a BUDDY predictor beside the structural counts
 * of the sketches above -- the SIGN-style levels X, A^ X, A^2 X, ..., which the predictor combines per pair as x_t[u] (.) x_t[v].  This comment is THE definition;
 * tests/hop_feature_ref.py restates it.  Per parent graph g of a store, with N nodes and feature width F = feat_dim:
 *   operator     the project's own GraphConv normalisation (the weighted-store comment above: norm(v) * sum w_uv * norm(u) * x[u]) over the WHOLE graph's in-edge
 *                CSR as the store holds it -- NOT the neighbour index: parallel edges count with their multiplicity, self loops count, directions are kept,
 *                weights are used on weighted stores.
 *   row of v     its in-CSR entries (u, w_uv) in stored order; w = 1.0f on unweighted stores.  Under GM_PROP_SELF_LOOPS (flag bit 1) one extra entry (v, 1.0f)
 *                stands in FRONT of every row: the A^ = D~^-1/2 (A + I) D~^-1/2 of GCN / SIGN / BUDDY.
 *   degree       d(v) = the fp32 sum of the row's weights in row order;  norm(v) = 1 / sqrtf(d(v) > 0 ? d(v) : 1).
 *   levels       x_0 = the store's feature rows.  For t = 0 .. hops - 1, in fp32:
 *                  x_{t+1}[v][f] = norm(v) * S,  S = the sum over the row's entries, in row order, of (w_uv * norm(u)) * x_t[u][f]
 *                where the coefficient c = w_uv * norm(u) is one fp32 product and S is accumulated from +0 as S = fmaf(c, x_t[u][f], S).  A row without entries
 *                gives zeros, as GraphConv does.  hops in 1 .. 8.
 *   hub rows     a row of more than C entries is summed in segments of C entries, each from +0, and the partial sums are added in ascending order (the first
 *                plus the second, plus the third, ...); its degree sum goes the same way.  C = gm_set_tuning("prop_chunk", C) / GM_PROP_CHUNK, 0 = the
 *                library's choice (256); the self-loop entry counts as an entry of its row.  The ORDER of a row sum, hence its low bits, belongs to C, as it
 *                does for ppr_chunk.  No float atomics, nothing depends on arrival order.
 *   exactness    for one value of prop_chunk the result is bit for bit a function of (graph, features, hops, flags) alone: not of the stream, not of how columns
 *                are tiled over lanes or workgroups, not of the zero padding of the store's row stride.  Column f of every level depends on column f of the
 *                features alone.  A weighted store with all weights 1.0 gives the unweighted bits.  Level 0 is STORED, equal to the store's features bitwise:
 *                the handle holds no pointer into the store, and destroying the store first is legal.
 *   pair rows    gm_prop_pair_features: d_pairs device int32 [n, 2], any orientation, a == b allowed;  d_out[k, t, f] = x_t[a][f] * x_t[b][f] (GM_PROP_HADAMARD) or
 *                fabsf(x_t[a][f] - x_t[b][f]) (GM_PROP_ABS_DIFF) for t = 0 .. hops: ONE fp32 operation on the rows gm_prop_rows returns, hence the same bits as
 *                that operation in numpy float32, and the same for both orientations.  A pair with a node outside [0, N) gives zeros.
 *   no mask flag the levels describe the WHOLE graph, as the sketches do: a pair's own edge cannot be taken out of them.
 *   memory       a handle owns (hops + 1) * N * ld * 4 bytes in one allocation, ld = the store's feature row stride (F where F is a multiple of 4, else F padded
 *                with zero columns to 32 or to a multiple of 64), laid out level-major, then node-major.  gm_set_tuning("prop_mib", M) / GM_PROP_MIB is the budget of one build in MiB, 0 = the library's
 *                choice, 8 GiB: GM_ERANGE (the message names N, hops, F, the bytes and the budget) when the formula exceeds it.
 * gm_store_propagate_build runs on `stream`, reads the graph's row lengths back once to cut the hub rows, takes the norms, the per-entry coefficients and the hub
 * segments' partial rows from the stream-ordered pool, and returns after the stream has produced every level: any stream may read them afterwards.
 * gm_prop_rows returns the rows of m nodes at one level, d_out: device float [m, F], dense (the padding columns never leave); duplicates are allowed, a node outside
 * [0, N) gives a row of zeros, nothing behind row m - 1 is written.  Both readers run on `stream` and are complete in stream order; m == 0 / n == 0 is a no-op, with
 * NULL pointers too.  gm_prop_dims fills whichever of its outputs is not NULL (bytes: the formula above).  gm_prop_destroy waits for the device and frees the levels.
 * GM_EINVAL (the message names the value): a bad graph index, hops outside 1 .. 8, unknown flag bits, an unknown op, a level outside 0 .. hops, m or n negative or
 * above INT32_MAX, a NULL argument with work to do, a negative prop_chunk or prop_mib.  GM_ERANGE: a build beyond prop_mib, a prop_chunk that cuts more than
 * 2^25 segments, a call whose launch would pass 2^31 workgroups. */
#define GM_PROP_SELF_LOOPS 1
#define GM_PROP_HADAMARD 0
#define GM_PROP_ABS_DIFF 1
typedef struct gm_prop gm_prop_t;
int32_t gm_store_propagate_build(const gm_store_t* s, int32_t g, int32_t hops, int32_t flags, void* stream, gm_prop_t** out);
int32_t gm_prop_dims(const gm_prop_t* p, int64_t* n_nodes, int32_t* hops, int32_t* feat_dim, int32_t* flags, int64_t* bytes);
int32_t gm_prop_rows(const gm_prop_t* p, int32_t level, const int32_t* d_nodes, int64_t m, float* d_out /* [m, F] */, void* stream);
int32_t gm_prop_pair_features(const gm_prop_t* p, const int32_t* d_pairs, int64_t n, int32_t op, float* d_out /* [n, hops + 1, F] */, void* stream);
void gm_prop_destroy(gm_prop_t* p);

/* ---- THE BUDDY PAIR PREDICTOR on those levels (beyond the reference): one hidden layer over the concatenation of a pair's level products and S caller-supplied
 * structure columns, scored and differentiated on the device without the [n, K] input matrix ever standing in memory.  This comment is THE definition;
 * tests/pair_mlp_ref.py restates it in float64.  For a handle p (levels x_0 .. x_hops, width F), a pair k = (a, b), op = GM_PROP_HADAMARD / GM_PROP_ABS_DIFF and
 * the columns s_k of d_extra (device float [n, S], dense, S >= 0; NULL where S == 0):
 *   z_k   = [ op(x_0[a], x_0[b]) | ... | op(x_hops[a], x_hops[b]) | s_k ]          K = (hops + 1) F + S;  op is the ONE fp32 operation of gm_prop_pair_features
 *   h_k   = relu(z_k W1 + b1)                                                      W1 [K, Hd], in x out, row-major (the GraphConv convention)
 *   l_k   = h_k . w2 + b2                                                          the logit
 *   loss  = (1/n) sum_k  max(l_k, 0) - l_k y_k + log1p(exp(-|l_k|))                y_k in [0, 1]: d_labels, device float [n]
 *   dl_k  = (sigmoid(l_k) - y_k) / n
 *   dw2 = sum dl_k h_k,  db2 = sum dl_k,  dh_k = dl_k w2 [h_k > 0],  dW1 = sum z_k (x) dh_k,  db1 = sum dh_k
 *   params       d_params and d_grad are ONE flat fp32 device buffer each, [W1 row-major | b1 | w2 | b2], n_params = K Hd + 2 Hd + 1 floats.
 *   limits       1 <= Hd <= 256, 0 <= S <= 256, any F / hops the handle holds, 0 <= n <= INT32_MAX.  Sizes that are no multiple of a tile are padded inside the
 *                kernels, never by the caller.  No gradient flows to the levels or to the structure columns: they are precomputed.
 *   nodes        a pair with a node outside [0, N) has zeros for its level columns, as in gm_prop_pair_features (its structure columns still count).
 *   arithmetic   every product carries both operands' full 24-bit significands (v_mfma_f32_32x32x2_f32: an fmaf chain per output); the sums are fp32.
 *   exactness    l_k is bit for bit a function of (levels, a, b, op, s_k, params) alone, with (a, b) and (b, a) equal: not of n, of the pair's place in the call,
 *                of the other pairs, of the stream, of pair_mlp_rows, and the same from gm_prop_pair_mlp_forward and gm_prop_pair_mlp_step -- a row's K order is
 *                fixed by the tile code.  The loss and the gradients are sums over pairs without float atomics: partial sums of fixed row ranges added in
 *                ascending order, the same bits for the same inputs and the same pair_mlp_rows.  gm_set_tuning("pair_mlp_rows", R) / GM_PAIR_MLP_ROWS: pairs
 *                per chunk of a step (0 = the library's choice, 65536), which bounds the dh scratch (R rows of Hd padded to 64 floats) and is the ONLY thing
 *                that may change the order of those sums, the role prop_chunk plays for the levels.
 * gm_prop_pair_mlp_dims fills K and n_params (either may be NULL); gm_prop_pair_mlp_tile returns the pair tile T of the kernels (a workgroup scores T pairs).
 * gm_prop_pair_mlp_forward stores the n logits.  gm_prop_pair_mlp_step stores the loss ([1]), the gradient ([n_params], OVERWRITTEN, never accumulated) and,
 * where d_logits is not NULL, the logits; with n == 0 it stores loss 0 and a zero gradient.  Both run on `stream`, take their scratch from the stream-ordered pool
 * and are complete in stream order; nothing outside [n] / [1] / [n_params] is written.
 * GM_EINVAL (the message names the value) before any launch: a NULL handle, Hd outside 1 .. 256, S outside 0 .. 256, an unknown op, n negative or above INT32_MAX,
 * a NULL argument with work to do (d_extra only where S > 0; d_logits of a step may be NULL), a negative pair_mlp_rows. */
int32_t gm_prop_pair_mlp_dims(const gm_prop_t* p, int32_t S, int32_t Hd, int32_t* K, int64_t* n_params);
int32_t gm_prop_pair_mlp_tile(void);
int32_t gm_prop_pair_mlp_forward(const gm_prop_t* p, const int32_t* d_pairs, int64_t n, int32_t op, const float* d_extra /* [n, S] */, int32_t S, const float* d_params,
                                 int32_t Hd, float* d_logits /* [n] */, void* stream);
int32_t gm_prop_pair_mlp_step(const gm_prop_t* p, const int32_t* d_pairs, int64_t n, int32_t op, const float* d_extra /* [n, S] */, int32_t S, const float* d_labels /* [n] */,
                              const float* d_params, int32_t Hd, float* d_logits /* [n], may be NULL */, float* d_loss /* [1] */, float* d_grad /* [n_params] */, void* stream);

/* ---- RANK COUNTS AND RANKING METRICS of device-resident scores (beyond the reference): the last stage of link prediction -- Hits@K, MRR and AUC of P positive
 * scores against negative scores, from exact integer counts formed on the device; a few integers and one double leave it.  This comment is THE definition;
 * tests/ranking_ref.py restates it by direct comparison.  d_pos: device float [P], d_neg: device float [N], d_neg_range: device int64 [P, 2] or NULL.
 *   order        scores are compared as IEEE fp32 VALUES: -0.0 == +0.0, denormals are distinct values and never flushed, +-inf are ordinary values.  The
 *                comparison runs on order-preserving integer keys, so the denormal mode of the device cannot matter: with u the bits of a score,
 *                u = 0 where u == 0x80000000 (-0.0 -> +0.0), then key = u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000); a < b as floats iff key(a) < key(b) as uint32.
 *   ranges       positive i is ranked against all N negatives where d_neg_range == NULL (the SHARED mode: the Hits@K protocol of ogbl-collab / -ppa / -ddi), else
 *                against d_neg[b_i .. e_i) with (b_i, e_i) = d_neg_range[i] (the MRR protocol of ogbl-citation2).  Ranges may be empty, overlap and repeat.
 *                N_i = the length of i's range (N in the shared mode).
 *   counts       d_counts[i] = (gt_i, eq_i): the negatives of the range strictly greater than d_pos[i], and those equal to it.  Exact integers, a function of
 *                d_pos[i] and the multiset of negatives in the range alone: not of P, of the other positives, of the order of the negatives, of the stream, or
 *                of any tuning value.
 *   summary      n_pos = P;  n_pairs = sum_i N_i;
 *                hits[j] = the number of positives with gt_i + eq_i < h_ks[j]  (OGB's pos > k-th largest negative; a positive with N_i < K is a hit);
 *                rr_sum  = sum_i 1 / (1 + gt_i + eq_i / 2) in fp64: the reciprocal of the mean of the optimistic and the pessimistic rank, exact in fp64, one
 *                          IEEE division per positive.  Summed without float atomics: partial sums over fixed ranges of i, added in a fixed ascending order that
 *                          belongs to P alone -- the same inputs give the same bits;
 *                auc2    = sum_i (2 (N_i - gt_i - eq_i) + eq_i): twice the Mann-Whitney U, an exact integer.
 *                The metrics are formed by the caller: hits@K = hits[j] / P,  mrr = rr_sum / P,  auc = (auc2 / 2.0) / (double)n_pairs.
 *   paths        the shared mode either sweeps the negatives per positive or sorts their keys once and searches them; gm_set_tuning("rank_sort_min", v) /
 *                GM_RANK_SORT_MIN: the N at or above which it sorts, 0 = the library's choice, 1 = always, INT32_MAX = never.  The integers are the same.
 * gm_rank_counts stores the [P, 2] counts.  gm_rank_summary reduces them on the device into *h_out (host) for the n_k values of h_ks (host); where d_counts is
 * not NULL it stores the counts too.  Both run on `stream`, take their scratch from the stream-ordered pool, write nothing outside [P, 2] and *h_out, read one
 * record back and return after the stream has produced the result.  P == 0: GM_OK, a zero summary, nothing else is looked at.
 * GM_EINVAL (the message names the value), before any launch: P or N negative or above INT32_MAX, n_k outside 0 .. GM_RANK_MAX_K, an h_ks[j] < 1, a NULL argument
 * with work to do (d_neg may be NULL where N == 0; d_counts of the summary may be NULL), a negative rank_sort_min.  Found on the device, in the pass that forms
 * the keys, and returned after the one read-back: a range with b < 0, e < b or e > N (no kernel walks a range of such a call), a NaN in either array.  On an
 * error the contents of d_counts are unspecified and *h_out is untouched.  GM_ERANGE: P * N above 2^61 (n_pairs could pass it). */
#define GM_RANK_MAX_K 8
typedef struct gm_rank_summary { int64_t n_pos, n_pairs, auc2; double rr_sum; int64_t hits[GM_RANK_MAX_K]; } gm_rank_summary_t;
int32_t gm_rank_counts(const float* d_pos, int64_t P, const float* d_neg, int64_t N, const int64_t* d_neg_range /* [P, 2] or NULL */, int64_t* d_counts /* [P, 2] */,
                       void* stream);
int32_t gm_rank_summary(const float* d_pos, int64_t P, const float* d_neg, int64_t N, const int64_t* d_neg_range /* [P, 2] or NULL */, const int64_t* h_ks, int32_t n_k,
                        int64_t* d_counts /* [P, 2], may be NULL */, gm_rank_summary_t* h_out, void* stream);

/* ---- Extraction: replaces Subgraphs.generate_subgraph / generate_subgraph_link_pred
 * (sdp.py:295-346: h-hop in-neighbour expansion, node sampling, G.subgraph) and dgl.batch
 * (sdp.py:399-406) for n_sets sets at once.  seeds/set_offsets are host arrays; set s owns seeds
 * [set_offsets[s], set_offsets[s+1]).  Nodes inside a subgraph are in ASCENDING parent id.  If a
 * neighbourhood has more than sample_nodes nodes, sample_nodes of them are kept by a keyed
 * permutation of (rng_seed, graph, i, j) and the centre(s) re-added (sdp.py:312-314,337-339).
 * link_pred is a MODE (gm_extract and gm_extract_pair; any other value is GM_EINVAL):
 *   0                  node seeds (j = -1): the h-hop in-neighbourhood of i, h in {1,2,3}.
 *   1                  pairs as the reference builds them: i side 2 hops, j side 1 hop, h IGNORED
 *                      (generate_subgraph_link_pred with its sdp.py:332 slip).  Two centres per subgraph.
 *   GM_LINK_SYMMETRIC  pairs, beyond the reference: {v : in-hop distance to i <= h} U {v : in-hop distance
 *                      to j <= h}, h in {1,2,3} (GM_EINVAL otherwise).  Same sampling key, same
 *                      threshold, both centres re-added; everything derived from the node set (node
 *                      order, both CSR orientations, centre indices, norms, GM_F_*) as in mode 1.
 * gm_batch_from_nodes takes the node sets as given and only asks whether there are two centres:
 * any non-zero link_pred means pairs (bit 2, GM_LINK_MASK_TARGET, aside: it is read as the mask).
 * GM_LINK_MASK_TARGET is a FLAG, OR-ed onto a pair mode (valid link_pred values: 0, 1, 2, 1|4, 2|4; the
 * flag alone is GM_EINVAL -- node seeds have no target link), beyond the reference: the subgraph of a
 * pair (i, j) is built WITHOUT the link it is asked about, as SEAL removes the target link from the
 * enclosing subgraph (an existing i-j edge otherwise tells the head the answer: j is a source of row i,
 * and label_j(i) == 1 under gm_set_hop_labels).  Under the flag, per subgraph with centres i, j:
 *   node set   the one the unmasked mode gives: the expansion runs on the unmasked parent, same sampling
 *              key (seed, g, i, j), same threshold, both centres re-added -- k hops first, then the link
 *              removed.  (Remark: in both pair modes that is also the expansion on the masked graph --
 *              whatever i reaches through j within h hops lies within h - 1 hops of j, and j's side is
 *              expanded too.  The definition is "unmasked node set".)
 *   edges      absent from the induced subgraph, in both CSR orientations (GM_F_INDPTR / GM_F_INDICES
 *              and the _T pair): every parent edge i -> j and every edge j -> i, all parallel copies
 *              included; for i == j every self loop i -> i.  No other edge changes, and the surviving
 *              edges of a row keep the parent's order.
 *   weights    the surviving edges carry their own weights at their new slots (GM_F_EDGE_W / _T).
 *   norm       in_deg.clamp(1)^-1/2 of the MASKED degree; weighted batches: of the masked weighted
 *              degree, summed in edge order.  A centre whose only in-edge was the target has norm 1.
 *   derived    hop labels (for i != j, label_j(i) and label_i(j) are never 1) and every finalisation
 *              table come from the masked CSR.
 *   no-op      a pair with no edge between its endpoints yields the unmasked subgraph bit for bit.
 * gm_batch_mask_target: 1 for a batch built under the flag, else 0; gm_batch_concat takes parts that are
 * all masked or all unmasked and hands the flag on.  Without the flag every field, launch and output is
 * what it was before the flag existed. */
#define GM_LINK_SYMMETRIC 2
#define GM_LINK_MASK_TARGET 4
int gm_extract(const gm_store_t* store, const gm_seed_t* seeds, int32_t n_seeds,
               const int32_t* set_offsets, int32_t n_sets, int32_t h, int32_t sample_nodes,
               uint64_t rng_seed, int32_t link_pred, void* stream, gm_batch_t** out);
/* The support AND the query batch of a meta-batch in one build (Subgraphs.__getitem__ extracts both per task, sdp.py:363-386; dgl.batch twice,
 * sdp.py:399-406): the same two batches two gm_extract calls return -- bit for bit -- from ONE launch of the node-set kernel and ONE of the fill
 * kernel over all subgraphs (a 32-task arxiv meta-batch: 288 + 2,304 of them) and one host round trip for both finalisations. */
int gm_extract_pair(const gm_store_t* store, const gm_seed_t* seeds_a, int32_t n_seeds_a, const int32_t* set_offsets_a, int32_t n_sets_a,
                    const gm_seed_t* seeds_b, int32_t n_seeds_b, const int32_t* set_offsets_b, int32_t n_sets_b,
                    int32_t h, int32_t sample_nodes, uint64_t rng_seed, int32_t link_pred, void* stream,
                    gm_batch_t** out_a, gm_batch_t** out_b);
/* Same, but the node set of every subgraph is given (host, ascending, concatenated; subgraph k
 * owns nodes_flat[nodes_off[k]..nodes_off[k+1])): G.subgraph(nodes) + dgl.batch only.  Used to
 * replay node sets sampled elsewhere (e.g. by the reference's numpy RNG). */
int gm_batch_from_nodes(const gm_store_t* store, const gm_seed_t* seeds, int32_t n_seeds,
                        const int32_t* set_offsets, int32_t n_sets, const int32_t* nodes_flat,
                        const int64_t* nodes_off, int32_t link_pred, void* stream, gm_batch_t** out);
/* HOP-DISTANCE LABELS, gm_set_hop_labels(D): off (0) by default, per calling thread (like gm_set_ragged_classes), D in 1..7 (anything outside 0..7
 * is ignored and leaves an error string); read by gm_extract, gm_extract_pair and gm_batch_from_nodes when they build a batch -- the labelling
 * step of local-subgraph methods (SEAL, distance encoding), beyond the reference.  Per subgraph and per centre c (one for node seeds, two -- i, j --
 * for pairs), with the BATCH's own induced in-edge CSR (GM_F_INDPTR / GM_F_INDICES, i.e. after sampling):
 *   d_c(v)     = the least k >= 0 such that a directed path v -> ... -> c of k edges lies inside the subgraph (BFS from c along in-edges);
 *   label_c(v) = d_c(v) if d_c(v) <= D, else D + 1 (farther rows and unreachable ones, e.g. where sampling cut the path);
 *   distances are topological: edge weights, parallel edges and self loops do not change them;
 *   Lw = D + 2 columns per centre;  x'(v) = [x(v) | onehot_Lw(label_i(v)) | onehot_Lw(label_j(v))] (second block: pairs only; a pair with
 *   i == j gets two identical blocks), so a model for a labelled batch has dims[0] = feat_dim + centres * Lw.  Labels are constants (no gradient).
 * GM_F_HOP exposes the labels; the batch owns its [rows, ld'] table of x' rows (ld' = the padded width, rows * ld' * 4 bytes of HBM per batch)
 * and every layer-1 gather of every schedule reads it through identity row tables (it no longer reads the store's cache-resident table), while
 * GM_F_FEAT_ROW keeps meaning the store row.  gm_gather_features returns x'.  A model whose dims[0] is not the batch's feature width is GM_EINVAL
 * (the message names both).  gm_set_split_pieces(2) is ignored on labelled batches (three pieces, violation word 0): the layer-1 operand bound
 * does not cover the 1.0 entries.  With the switch off every batch field, launch and output is what it was without the feature.
 * gm_batch_hop_labels: the batch's D, or 0. */
void gm_set_hop_labels(int32_t D);
int32_t gm_get_hop_labels(void);
int32_t gm_batch_hop_labels(const gm_batch_t* b);
int32_t gm_batch_mask_target(const gm_batch_t* b);
/* dgl.batch over already-built batches (sets are appended in order).  Inputs stay valid.  Parts of one store are all weighted or all
 * unweighted; a mix (hand-made handles) is GM_EINVAL.  Parts are all hop-labelled with the same D, or all unlabelled (a mix: GM_EINVAL); the result's
 * feature table is the concatenation of the parts'.  Parts are all built with GM_LINK_MASK_TARGET or all without (a mix: GM_EINVAL); the result
 * carries the flag. */
int gm_batch_concat(const gm_batch_t* const* parts, int32_t n_parts, void* stream, gm_batch_t** out);
/* Receptive-field tables for gm_hparams_t.cone with an n_gcn-layer model (built on `stream`, cached in the
 * batch; gm_meta_ws_bytes/gm_meta_step build them on first use otherwise).  level_rows/level_edges
 * (host int64[n_gcn+1]): rows of level l and edges from level l-1 into level l; *ok = 0 when the batch
 * cannot use the schedule.  gm_batch_cone_read copies one table to the host (tests): what = 0 rows,
 * 1 indptr, 2 indices, 3 indptr_t, 4 indices_t, 5 set offsets. */
int gm_batch_prepare_cone(const gm_batch_t* b, int32_t n_gcn, void* stream);
/* The same for the two batches of a meta-batch (support, query) with ONE pair of host round trips for both
 * (the builder thread of Subgraphs.batches calls this; results identical to two gm_batch_prepare_cone calls). */
int gm_batch_prepare_cone_pair(const gm_batch_t* a, const gm_batch_t* b, int32_t n_gcn, void* stream);
int gm_batch_cone_dims(const gm_batch_t* b, int32_t n_gcn, int32_t* ok, int64_t* level_rows, int64_t* level_edges);
int gm_batch_cone_read(const gm_batch_t* b, int32_t n_gcn, int32_t level, int32_t what, void* host, int64_t host_bytes);
void gm_batch_destroy(gm_batch_t* b);

/* Sizes: rows = total nodes, edges = total induced edges, subs = subgraphs, sets = task sets,
 * centres = 1 (node-clf) or 2 (link-pred). */
int gm_batch_dims(const gm_batch_t* b, int64_t* rows, int64_t* edges, int32_t* subs, int32_t* sets,
                  int32_t* centres);
enum gm_field {
    GM_F_SUB_OFF = 0,   /* int32[subs+1]  row offset of each subgraph == cumsum(batch_num_nodes) (learner.py:161-163) */
    GM_F_SET_SUB_OFF,   /* int32[sets+1]  subgraph range of each set                                                */
    GM_F_PARENT,        /* int32[rows]    parent node id of each row == sub.parent_nid (sdp.py:317)                  */
    GM_F_GRAPH,         /* int32[subs]    parent graph of each subgraph                                              */
    GM_F_INDPTR,        /* int32[rows+1]  in-edge CSR of the batched induced graph                                   */
    GM_F_INDICES,       /* int32[edges]   source ROW of every in-edge                                                */
    GM_F_INDPTR_T,      /* int32[rows+1]  by-source CSR (for the backward aggregate)                                 */
    GM_F_INDICES_T,     /* int32[edges]   destination ROW of every out-edge                                          */
    GM_F_CENTRE,        /* int32[subs*centres] local index of the centre(s) inside each subgraph (sdp.py:318-319)    */
    GM_F_NORM,          /* float[rows]    in_degree.clamp(1)^-0.5 (learner.py:29); weighted batches: the weighted in-degree      */
    GM_F_FEAT_ROW,      /* int32[rows]    row of the store's feature matrix for each batch row (also on hop-labelled batches) */
    GM_F_NORM_SRC,      /* float[rows]    GM_F_NORM with the sign bit set on every row without an out-edge inside the batch: no later
                                          kernel reads that row of a hidden activation below the last layer (GM_DEAD_ROWS)       */
    GM_F_NORM_CENTRE,   /* float[rows]    GM_F_NORM with the sign bit set on every row that is not a centre                     */
    GM_F_EDGE_W,        /* float[edges]   weight of every in-edge, aligned with GM_F_INDICES (weighted batches only: GM_EINVAL otherwise) */
    GM_F_EDGE_W_T = 14, /* float[edges]   the same weights in the order of GM_F_INDICES_T (weighted batches only)                       */
    GM_F_HOP = 15,      /* int8[rows*centres] hop-distance label of every row per centre, row-major [rows, centres] (hop-labelled batches only: GM_EINVAL otherwise) */
    GM_F_NORM_E1 = 16,  /* float[rows]    GM_F_NORM with the sign bit set on every row that is not the source of an in-edge of a centre: the last
                                          layer's backward leaves the gradient of the layer below zero there (GM_DEAD_ROWS=2)     */
    GM_F_EDGE_CENTRE_T = 17,/* int32[edges] per edge of GM_F_INDICES_T: the destination row where it is a centre, else `rows` -- the zero row the
                                          dense backward keeps behind its [rows, width] product T (GM_DEAD_ROWS=2)                 */
    GM_F_OBS_CENTRE = 18, /* float[rows]  +1 on the centre rows, -1 on every other row: the keep flag (a scale of exactly 1) of the last layer's partial
                                          aggregate in a pass nobody differentiates (GM_DEAD_ROWS=3) and in a differentiated pass (4) */
    GM_F_OBS_E1 = 19    /* float[rows]    +1 on the sources of the centres' in-edges (the rows GM_F_NORM_E1 keeps), -1 on every other row: the same
                                          flag for the layer below the last (GM_DEAD_ROWS=3, 4)                                    */
};
int32_t gm_batch_weighted(const gm_batch_t* b);
/* Copies a field to host memory (synchronises `stream` internally). */
int gm_batch_read(const gm_batch_t* b, int32_t field, void* host_dst, int64_t bytes);
/* Device address of a field (valid until gm_batch_destroy). */
int gm_batch_device_ptr(const gm_batch_t* b, int32_t field, void** dptr);
/* Rows with at least one out-edge inside the batch: the rows of GM_F_NORM_SRC whose sign bit is clear. */
int gm_batch_source_rows(const gm_batch_t* b, int64_t* n_rows);
/* Distinct source rows of the centres' in-edges: the rows of GM_F_NORM_E1 whose sign bit is clear (synchronises the batch's stream at first use). */
int gm_batch_e1_source_rows(const gm_batch_t* b, int64_t* n_rows);

/* ---- Feature gather: replaces np.vstack([feat[g][ids] ...]) + H2D (meta.py:119-120,193-194).
 * x_out: device fp32 [rows, feat_dim]; hop-labelled batches: [rows, feat_dim + centres * (D + 2)], the labelled rows x'. */
int gm_gather_features(const gm_batch_t* b, float* x_out, void* stream);

/* ---- GCN building blocks (GraphConv.forward, learner.py:25-56), exported for tests/profiling.
 * out[v,:] = s_out[v] * sum_{u in row v} s_in[u] * x[u,:]   (s_in / s_out may be NULL = 1).
 * transposed != 0 runs on the by-source CSR (autograd backward of update_all).  If gather != 0,
 * x is ignored and rows are read from the store's features through GM_F_FEAT_ROW.
 * Weighted batches: every term also carries w_uv.  s_in == NULL sums w_uv * x[u]; s_in == the batch's own GM_F_NORM device pointer sums
 * w_uv * norm[u] * x[u]; any other s_in is GM_EINVAL (the per-source gather has no weight slot), and so is gather with transposed. */
int gm_aggregate(const gm_batch_t* b, int32_t transposed, int32_t gather, const float* x, int32_t width,
                 const float* s_in, const float* s_out, float* out, void* stream);
int64_t gm_aggregate_bytes(const gm_batch_t* b, int32_t width); /* algorithmic HBM bytes of one call */

/* ---- Classifier.forward / backward (learner.py:134-175) for a batch whose set s uses the
 * parameter vector params + s*param_stride (param_stride = 0: every set shares one vector, the
 * `vars=None` case).  x0: device [rows, dims[0]] or NULL (gather from the store).
 * centre_local: device int32 [subs*centres] `to_fetch` override or NULL (use the batch's own).
 * logits: device fp32 [subs, n_out].  ws must hold gm_gcn_ws_bytes(); it carries the activations
 * from forward to backward (pass the same x0 / centre_local to both).  dlogits: device [subs, n_out];
 * dparams: device, set s written at dparams + s*dparam_stride (dparam_stride >= P).
 * params + s*param_stride must be 16-byte aligned for the vectorised weight loads (else a scalar path runs). */
int64_t gm_model_param_count(const gm_model_t* m);
int64_t gm_gcn_ws_bytes(const gm_batch_t* b, const gm_model_t* m);
int gm_gcn_forward(const gm_batch_t* b, const gm_model_t* m, const float* params, int64_t param_stride,
                   const float* x0, const int32_t* centre_local, float* logits, void* ws, int64_t ws_bytes,
                   void* stream);
int gm_gcn_backward(const gm_batch_t* b, const gm_model_t* m, const float* params, int64_t param_stride,
                    const float* x0, const int32_t* centre_local, const float* dlogits, float* dparams,
                    int64_t dparam_stride, void* ws, int64_t ws_bytes, void* stream);

/* torch.matmul(feat, weight) of GraphConv.forward (learner.py:36,47) over the rows of a batch: out[rows, N] = x[rows, K] @ W_t with
 * W_t = W + set * w_stride ([K, N] row-major; w_stride = 0: one matrix for every set).  Exported for numerics tests of the GEMM kernels.
 * mode -1: what the library would pick (gm_set_gemm_mode + launch size), 0: exact-fp32 MFMA kernels, 1: split-bf16 kernel (three pieces, N = 128 / 256),
 * 2: split-fp16 kernel (two pieces; the bounds of x and of every W_t are taken by the call itself). */
int gm_dense_update(const gm_batch_t* b, const float* x, int32_t K, const float* W, int64_t w_stride, int32_t N, float* out, int32_t mode,
                    void* stream);
/* The same product with the epilogue of the forward and dZ GEMMs, exported for numerics tests of every kernel gm_dense_update can reach:
 *   out[r, :N] = epi(s[r] * (x[r, :K] @ B_t) + bias_t)   for the rows r of set t,
 * B_t = W_t ([K, N] row-major), or W_t^T when trans_w (W_t stored [N, K], as in dZ = dQ W^T);  W_t = W + t * w_stride (0: one matrix for every
 * set);  x: device [rows, ldx];  out: [rows, ldc], columns [N, ldc) untouched.  s: row scale [rows] or NULL (1); s_keep (split kernels only,
 * or NULL): the row scale again with the sign bit set on rows that are computed and not stored (the exact kernels use s and store every row);
 * bias_t = bias + t * bias_stride [N] or NULL;  relu: max(v, 0), NaN kept.  relu_bits (or NULL): packed relu' bits of the stored value, byte
 * (r * ldc + c) / 4, bit c % 4;  mask_h [rows, ldc] (or NULL): zero where mask_h <= 0;  mask_b (or NULL): the same as packed bits.
 * zero_out (or NULL): a [rows, ldc] buffer filled with zeros (the split kernels need ldc == N).  amax_out (mode 2 only, or NULL): per-set slots
 * t * 64 (zeroed by the caller) that receive the fp32 bits of the largest |out| the kernel stores for set t.
 * mode -1: the library's choice (gm_set_gemm_mode + launch size; three pieces), 0: exact-fp32 kernels (by shape and alignment), 1: split-bf16
 * kernel (three pieces), 2: split-fp16 kernel (two pieces; per-set bounds of x's rows and of every W_t are taken by the call itself).
 * GM_EINVAL: a split kernel with mask_h / mask_b, N not 128 or 256, K not a multiple of 16 or below 32, or zero_out with ldc != N;
 * relu_bits / mask_b where the C stores are not 16-byte vectors.  launched (or NULL) receives the id of the kernel instantiation that ran
 * (GM_GEMM_ID_* in the library's internal header). */
int gm_dense_gemm(const gm_batch_t* b, const float* x, int64_t ldx, int32_t K, const float* W, int64_t w_stride, int32_t trans_w, int32_t N,
                  float* out, int64_t ldc, const float* s, const float* s_keep, const float* bias, int64_t bias_stride, int32_t relu,
                  uint8_t* relu_bits, const float* mask_h, const uint8_t* mask_b, float* zero_out, uint32_t* amax_out, int32_t mode,
                  int32_t* launched, void* stream);
/* The fused aggregate + GEMM of a forward pass, exported for numerics tests: gm_dense_gemm's split kernels with the A operand formed in the loader,
 *   Z[r] = w0 * X[u0] + w1 * X[u1]  from the batch's per-row source table {u0, u1, w0, w1} (gm_dense_agg_table 4 / 5),  out = epi(s (Z @ W_t) + bias_t).
 * table 0: X = x [rows, ldx], sources are batch rows;  table 1: X = the batch's feature table (x, ldx ignored; K = its feature width, or its row stride).
 * The table is always the batch's own.  zside [rows, ldz]: the finished aggregate of the rows of more than two sources (the only rows of it that are read;
 * 16-byte aligned, ldz a multiple of 4).  mode 1: three pieces;  2: two pieces, with the per-set bounds of A taken over zfull [rows, ldzf], a fully
 * aggregated Z (never over zside).  The other parameters are gm_dense_gemm's; launched receives the id of k_gemm_split_p<true, ...> (40, 41, 44, 45).
 * GM_EINVAL (nothing launched, no output touched): K below 64, a misaligned zside, ldz not a multiple of 4, and gm_dense_gemm's refusals. */
int gm_dense_fused_gemm(const gm_batch_t* b, int32_t table, const float* x, int64_t ldx, int32_t K, const float* zside, int64_t ldz, const float* zfull,
                        int64_t ldzf, const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc, const float* s, const float* s_keep,
                        const float* bias, int64_t bias_stride, int32_t relu, uint8_t* relu_bits, float* zero_out, uint32_t* amax_out, int32_t mode,
                        int32_t* launched, void* stream);
/* The same launch over the table of a row set, as the restricted forward-only layers run it (tests): rowset 0 the centre rows (table 7 of gm_dense_agg_table, keep
 * vector GM_F_NORM_CENTRE; table must be 0), 1 the sources of the centres' in-edges (table 8, or 9 with table == 1; GM_F_NORM_E1).  s = GM_F_NORM.  keep != 0: the
 * set's keep vector is the launch's s_keep (only its rows are stored); 0: every row is stored.  live_on != 0: the launch gets the set's tile flags (GM_DEAD_TILES;
 * gm_dense_agg_table 13 / 14): a tile without a kept row issues its MFMAs and nothing else -- taken by the three-piece kernel where keep is on and neither relu_bits
 * nor zero_out is given, ignored otherwise.  grid: workgroups of the launch (0: the library's rule; a small batch otherwise gets one tile per workgroup). */
int gm_dense_fused_gemm_rows(const gm_batch_t* b, int32_t rowset, int32_t keep, int32_t live_on, int32_t grid, int32_t table, const float* x, int64_t ldx, int32_t K,
                             const float* zside, int64_t ldz, const float* zfull, int64_t ldzf, const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc,
                             const float* bias, int64_t bias_stride, int32_t relu, uint8_t* relu_bits, float* zero_out, uint32_t* amax_out, int32_t mode,
                             int32_t* launched, void* stream);
/* ... over the row set's PACKED tiles (GM_PACK_ROWS; tests): keep and the tile flags on, three pieces, and the set's kept rows packed per set into the fewest tiles
 * (gm_dense_agg_table 15 .. 20).  The launch walks the same tiles per workgroup as gm_dense_fused_gemm_rows; the packed ones are fed and stored at their own rows,
 * every other tile issues its MFMAs alone.  The bytes of `out` are those of gm_dense_fused_gemm_rows with keep on, whatever live_on and grid. */
int gm_dense_fused_gemm_packed(const gm_batch_t* b, int32_t rowset, int32_t grid, int32_t table, const float* x, int64_t ldx, int32_t K, const float* zside, int64_t ldz,
                               const float* W, int64_t w_stride, int32_t N, float* out, int64_t ldc, const float* bias, int64_t bias_stride, int32_t relu,
                               int32_t* launched, void* stream);
/* One aggregate launch over one orientation of the batch (0: the in-edge CSR, transposed: the by-source CSR) with every option the library's own callers
 * set, exported for numerics tests of every aggregate kernel (agg.hip, agg_stream.hip):
 *   out[v, :width] = epi(|s_out[v]| * sum over the edges e of row v of w_e * X[src_e, :] + bias_t)      for the rows v of set t.
 * x_src: 0 X = x (device [rows, ldx]); 1 X = the batch's feature table through GM_F_FEAT_ROW per source; 2 the same through the per-edge row table (by-destination
 *   CSR only); 3 X = x read through GM_F_EDGE_CENTRE_T (transposed only; x holds rows + 1 rows, the last one zero).  1 and 2 need width == the feature width.
 * scale_src: 0 w_e = 1 (weighted batches: the edge's weight); 1 w_e = s_in[src_e], gathered per source (refused on weighted batches, as gm_aggregate does);
 *   2 w_e from the batch's per-edge table of GM_F_NORM[src_e] (weighted batches: weight x norm).  s_in is given with scale_src == 1 only.
 * s_out (or NULL): row scale; keep_signed: its sign bit marks rows that are not stored (computed where relu_bits are written -- the bits of every row are --,
 *   left alone otherwise), the scale is the magnitude.  bias_t = bias + t * bias_stride
 *   (stride 0: one bias for every set) or NULL;  relu: max(v, 0), NaN kept;  relu_bits (or NULL, with relu): packed relu' bits of the stored value, byte
 *   (v * width + c) / 4, bit c % 4;  mask_h [rows, width] (or NULL): zero where mask_h <= 0;  mask_b (or NULL): the same as packed bits.
 * hubs: 0 no hub handling (every row by the row kernels); 1 the batch's hub-row list without a schedule (a separate hub launch); 2 its block schedule and hub parts.
 * rowlist (device, ascending, n_list entries; or NULL): the windows walk these rows in windows of list_win rows (2, 4, .. 64); list_sched: with the batch's own
 *   schedule over its list of window rows (the list must be that list); list_sched 2 / 3 / 4 with rowlist NULL: the launch walks the batch's own list 0 / 1 / 2 of
 *   observable rows (gm_dense_obs_lists; 4 goes with transposed) as the model's launches do: sized by the list's bound, with its window and its own block schedule,
 *   the length read on the device.  skip_lo <= skip_hi: rows of those degrees are left unwritten (window kernel only).
 * stream_ok: the launch may take the stream kernel where the library's own callers could (hubs == 2, scale_src == 2, no epilogue option).
 * launched (or NULL) receives the id of the kernel instantiation that ran (GM_AGG_ID_* in the library's internal header).
 * GM_EINVAL: mask_h together with mask_b; a row list together with stream_ok, off the window kernel, not ascending or out of range; a gather of another width
 *   than the feature width; relu_bits / mask_b where the stores are not 16-byte vectors; on weighted batches scale_src 1 and x_src 1 (gm_aggregate's refusals: only
 *   the per-edge tables have a slot for the weights). */
int gm_dense_aggregate(const gm_batch_t* b, int32_t transposed, int32_t x_src, const float* x, int64_t ldx, int32_t width, int32_t scale_src,
                       const float* s_in, const float* s_out, int32_t keep_signed, const float* bias, int64_t bias_stride, int32_t relu,
                       uint8_t* relu_bits, const float* mask_h, const uint8_t* mask_b, int32_t hubs, const int32_t* rowlist, int64_t n_list,
                       int32_t list_win, int32_t list_sched, int32_t skip_lo, int32_t skip_hi, int32_t stream_ok, float* out, int32_t* launched,
                       void* stream);
/* What those tests need to know about one orientation of a batch: info[16] = {hub threshold, hub rows, rows per scheduled window, edges per hub part (0: unsplit),
 * hub parts, scheduled, rows of the batch's window-row list, its window, list schedule present, stream row segments (0 before the orientation's first
 * stream-eligible launch), stream workgroups, hub workgroups among them, weighted, feature width, feature row stride, 0};  gm_dense_fuse_counts: counts[2] = {rows
 * of more than two sources in the in-edge CSR (the rows a fused pass still aggregates by the ordinary kernel), their in-edges};  gm_dense_agg_table copies n entries of
 * a derived table to dst (device): which 0 per-edge source norm (float), 1 per-edge feature row, 2 window-row list, 3 hub rows (int32); 4 / 5 / 6 the per-row
 * source tables of the fused kernels, [rows] entries of four int32 {u0, u1, w0, w1} (w: fp32 bits): 4 sources as batch rows, 5 as rows of the feature table,
 * 6 the last layer's dQ table.  A source flagged 0x40000000 is the row's own finished row, 0x20000000 an all-zero row:
 *   no source {ZERO, ZERO, 1, 0};  one {u0, u0, w0, 0};  two {u0, u1, w0, w1};  more {row | SELF, row | SELF, 1, 0};  w = norm[u] (x the edge's weight);
 *   dQ table: a centre row {row | SELF, ZERO, 1, 0}, any other {ZERO, ZERO, 0, 0}.
 * 7 / 8 / 9 (GM_DEAD_ROWS=3; at 4 also of the differentiated passes and their weight gradients) the tables of the passes nobody differentiates, same layout: 7 table 4's entry on the centre rows, 8 table 4's and 9 table 5's
 * entry on the sources of the centres' in-edges (the rows GM_F_OBS_E1 keeps); every other row {ZERO, ZERO, 0, 0}.
 * 10 / 11 / 12 (int32, up to the list's bound) the ascending lists of observable rows that the restricted aggregate launches walk (GM_AGG_OBS_LIST): rows of 3 ..
 *   hub-threshold sources that GM_F_OBS_CENTRE keeps, the same that GM_F_OBS_E1 keeps, and every row GM_F_NORM_E1 keeps.  gm_dense_obs_lists: info[16], per list
 *   {length (read back at first use: synchronises the stream), the bound it is allocated and scheduled for, rows per window, 0 not taken / 1 taken / 2 nothing to
 *   launch, + 4 with a block schedule of its own}, then {observable rows of more than two sources (hub rows included) of the centre set, of the set GM_F_OBS_E1
 *   keeps (-1 without the tables), rows GM_F_NORM_E1 keeps, 0}.
 * 13 / 14 (int32, one per GEMM row tile of 128 rows inside a set, gm_batch_info's tile count) the tile flags of GM_DEAD_TILES: 1 where some row of the tile is kept
 *   by GM_F_NORM_CENTRE / GM_F_NORM_E1, else 0.
 * 15 .. 20 (int32; GM_PACK_ROWS) the same two row sets packed per set, ascending by row: 15 / 16 the packed row ids (up to the host's bound: per set its centres / the
 *   in-edges of its centres, capped by its rows; set t's entries start at the prefix of those bounds), 17 / 18 the packed tile tables, three words {set, offset into
 *   the packed arrays, rows <= 128} per tile (n counts words), 19 / 20 the number of packed tiles (one word): the sum over the sets of ceil(kept rows / 128). */
int gm_dense_obs_lists(const gm_batch_t* b, int64_t* info, void* stream);
int gm_dense_agg_info(const gm_batch_t* b, int32_t transposed, int64_t* info);
int gm_dense_fuse_counts(const gm_batch_t* b, int64_t* counts);
int gm_dense_agg_table(const gm_batch_t* b, int32_t which, int32_t transposed, void* dst, int64_t n, void* stream);
/* The last layer's dZ product and weight gradient where dQ holds its CENTRE rows only (GM_DEAD_ROWS: gm_meta_step no longer zero-fills the others;
 * their bytes may be anything), exported for tests:  T[r, :N] = norm[r] * (dQ0[r, :K] @ W_t^T)  with W_t stored [N, K] and dQ0 = dQ on the batch's
 * centre rows, 0 elsewhere -- through the fused split kernel and the batch's per-row table;  dW_t[Kx, N] = sum_r (norm[r] x[r, :Kx])^T dQ0[r, :N],
 * db_t[N] = sum_r dQ0[r, :N] -- through the split weight-gradient kernel's flagged-row variant.  Three pieces; dims as for modes 1 of gm_dense_gemm /
 * gm_dense_wgrad (K >= 64 here), GM_EINVAL otherwise. */
int gm_dense_dz_centre(const gm_batch_t* b, const float* dQ, int32_t K, const float* W, int64_t w_stride, int32_t N, float* T, void* stream);
/* gm_dense_dz_centre storing the centre rows of T only, with the centres' tile flags (GM_DEAD_TILES) and, pack != 0, over their packed tiles (GM_PACK_ROWS); grid:
 * workgroups (0: the library's rule).  The other rows of T are left as they are. */
int gm_dense_dz_centre_rows(const gm_batch_t* b, const float* dQ, int32_t K, const float* W, int64_t w_stride, int32_t N, float* T, int32_t pack, int32_t grid, void* stream);
int gm_dense_wgrad_centre(const gm_batch_t* b, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                          int64_t db_stride, void* stream);
/* One level down (GM_DEAD_ROWS=2), exported for tests: the last layer's transposed aggregate  out[u, :] = mask[u, :] ? norm[u] * sum over the out-edges
 * (u -> v) of w_uv T[v, :] : 0  as the dense backward launches it.  keep != 0: T is read through GM_F_EDGE_CENTRE_T -- its centre rows and one zero row
 * behind it (T holds rows + 1 rows of `width` floats; the call zeroes the last one, the others outside the centre rows may hold anything) -- and only the
 * rows GM_F_NORM_E1 keeps are worked on and stored: a row it flags has no reader in this launch and stops at its descriptor (no edge-table entry, no row
 * of T and no mask byte is loaded for it), its row of `out` is left untouched; keep == 0: the plain launch over every row of T.  mask_b: packed relu'
 * bits, byte (row * width + col) / 4, or NULL.  gm_dense_wgrad_e1 is gm_dense_wgrad_centre with GM_F_NORM_E1 as the flag. */
int gm_dense_agg_centre_t(const gm_batch_t* b, float* T, int32_t width, const uint8_t* mask_b, float* out, int32_t keep, void* stream);
int gm_dense_wgrad_e1(const gm_batch_t* b, const float* x, int32_t Kx, const float* dQ, int32_t N, float* dW, int64_t dw_stride, float* db,
                      int64_t db_stride, void* stream);
/* The weight gradient of the same layer (learner.py backward of `torch.matmul(feat, weight)` + bias) over the batch's weight-gradient row chunks,
 * per set t:  dW_t[K, N] = sum over the set's rows r of (s[r] x[r, :])^T g[r, :]  and  db_t[N] = sum_r gb[r, :].  Exported for numerics tests of the
 * weight-gradient kernels.  x: device [rows, ldx] (K used), g: [rows, ldg] (N used); s: row scale [rows] or NULL (1); gb: [rows, ldgb] or NULL (g).
 * dW_t = dW + t * dw_stride, db_t = db + t * db_stride (db may be NULL).  mode -1: what the library would pick (gm_set_gemm_mode + launch size;
 * three pieces), 0: exact fp32 (k_wgrad_fast or k_wgrad, by shape and alignment), 1: split-bf16 kernel (three pieces), 2: split-fp16 kernel (two
 * pieces; per-set bounds of x and g and one bound of |s| are taken by the call itself).  Modes 1 and 2 need K, N in {128, 256}, no gb and 16-byte
 * aligned x, g with ldx, ldg multiples of 4 (else GM_EINVAL); K or N above 2048: GM_ERANGE.  Optional fused inner SGD step (next != NULL):
 * parameter vectors cur_t / next_t = cur / next + t * p_stride laid out as W [K, N] then b [N]:  next_t = cur_t - lr * (dW_t, db_t);  wt (or NULL):
 * next_t's W transposed, [set][N][K];  pl_fwd / pl_dz (or NULL; K, N multiples of 32): next_t's W as three bf16 planes in the layouts of the
 * split GEMM's operands, [set][3][K/8][N][8] and [set][3][N/8][K][8]. */
int gm_dense_wgrad(const gm_batch_t* b, const float* x, int64_t ldx, int32_t K, const float* g, int64_t ldg, int32_t N, const float* s,
                   const float* gb, int64_t ldgb, float* dW, int64_t dw_stride, float* db, int64_t db_stride, int32_t mode,
                   const float* cur, float* next, int64_t p_stride, float lr, float* wt, uint16_t* pl_fwd, uint16_t* pl_dz, void* stream);
/* The same gradient over a Z whose forward ran fused, exported for numerics tests:  dW_t = sum_r (|s[r]| Z[r, :])^T g0[r, :],  db_t = sum_r g0[r, :],  with
 * Z[r] formed from gx through the batch's own per-row source table as in gm_dense_fused_gemm (table 0: gx [rows, ldgx];  1: the batch's feature table) and
 * read from A [rows, lda] only on the rows of more than two sources.  s: row scale or NULL;  g_keep (or NULL): the row scale again with the sign bit set on
 * the rows of g that nobody wrote -- they enter as zeros whatever their bytes hold (g0; without g_keep g0 = g), and |g_keep| scales Z in place of s.
 * mode 1: the three-piece split kernel (K, N in {128, 256}).  Modes 0 (exact kernels) and 2 (two-piece operands) cannot take a table: GM_EINVAL, no
 * output touched. */
int gm_dense_wgrad_fused(const gm_batch_t* b, int32_t table, const float* A, int64_t lda, int32_t K, const float* gx, int64_t ldgx, const float* g,
                         int64_t ldg, int32_t N, const float* s, const float* g_keep, float* dW, int64_t dw_stride, float* db, int64_t db_stride,
                         int32_t mode, void* stream);

/* ---- Prototypical losses (meta.py:28-54 proto_loss_spt, 56-79 proto_loss_qry), per set.
 * y: HOST int32 [subs] labels.  Outputs (device): loss[sets], acc[sets], protos[sets, c_task, n_out]
 * (c_task = the LARGEST number of classes of any set; every set keeps its own class layout -- classes, rows per class --
 * like the per-task calls of meta.py:118-157; set t uses the first classes_t rows of its [c_task, n_out] block),
 * dlogits[subs, n_out] (may be NULL), dprotos[sets, c_task, n_out] (qry only, may be NULL).
 * Every class of a set must score the same number of rows, and hold at least n_support of them on the support side (GM_EINVAL otherwise:
 * torch.stack at meta.py:42,65), unless the calling thread has switched on
 *
 * RAGGED-TASK MODE, gm_set_ragged_classes(1): off by default, per calling thread (like gm_last_error and the profile counters), honoured by
 * gm_proto_loss_spt / _qry, gm_meta_step and gm_meta_adapt.  Per task t:
 *   - classes C_t = the sorted unique SUPPORT labels; class c contributes its first min(n_support, count) support rows in batch order, n_c >= 1 of
 *     them; prototype p_c = the mean of the head outputs of those rows;
 *   - support loss / accuracy: over all sum_c n_c contributing rows, mean(-log_softmax(-|z - p|^2)[own class]) and the share of rows whose FIRST
 *     maximum of the fp32 log-probabilities is their own class;
 *   - query loss / accuracy: the same two means over ALL query rows of the task, each scored against the class its label has in C_t, rows visited
 *     class by class in sorted class order and in batch order inside a class (the fp32 summation order).  A support class may have no query rows; a
 *     query label outside C_t, or a task without query rows, is GM_EINVAL (the message names the task and the label);
 *   - these are SAMPLE means (`.view(-1).mean()`, meta.py:51,76) -- on a balanced task the reference's numbers; there is no class-balanced weighting;
 *   - backward: dL/dz of the query role is (softmax - onehot) / Q_t; the prototype role spreads dL/dp_c over the class's n_c support rows as / n_c;
 *   - limits: at most 256 classes and at most 8192 scored rows per set, else GM_ERANGE.
 * A set whose classes all score the same number of rows runs the same code as with the mode off, bit for bit.  The stand-alone gm_proto_loss_qry has
 * no support labels: there a set's classes are its own sorted labels, at most c_task of them, scored against the set's first prototypes. */
int gm_proto_loss_spt(const gm_batch_t* b, const float* logits, int32_t n_out, const int32_t* y, int32_t n_support,
                      float* loss, float* acc, float* protos, float* dlogits, void* stream);
int gm_proto_loss_qry(const gm_batch_t* b, const float* logits, int32_t n_out, const int32_t* y, const float* protos,
                      int32_t c_task, float* loss, float* acc, float* dlogits, float* dprotos, void* stream);
void gm_set_ragged_classes(int32_t on);     /* 1 / 0: ragged-task mode of the calling thread (above); workspace sizes depend on it */
int32_t gm_get_ragged_classes(void);
/* One launch of the classifier head with the prototypical loss (and the head's backward) as gm_meta_step issues it after the last GCN layer, exported for
 * numerics tests of k_head_loss and of the unfused k_head_fwd / k_proto / k_head_bwd.  The LDS sizing, the staging decision (GM_HEAD_STAGE, and unstaged
 * by itself above 150 KB of LDS per set), the workgroup size (GM_HEAD_THREADS) and the choice of the ragged instantiations are the library's own code.
 *   H: device fp32 [rows, Hd], the post-relu output of the last layer; compact != 0: [subs * nc, Hd], the centre rows only, in centre order.
 *   nc: centres per subgraph, the batch's own; with a compact H also 1 on a pair batch (pooled rows).  The head reads hc = nc * Hd columns, C = classes (<= 64).
 *   params + t * param_stride (0: one vector for every set): Wl [C, hc] at wl_off, bl [C] at bl_off.  centre_local: as gm_gcn_forward, or NULL.
 *   y: HOST int32 [subs].  mode 0: support loss over the first n_support rows of every class (protos_out [sets, classes, C] or NULL);  mode 1: query loss
 *   against protos [sets, c_task, C] (dprotos likewise, or NULL).  Class tables by the rules of gm_proto_loss_spt / _qry, ragged-task mode included; in that
 *   mode and mode 1, spt_labels / spt_counts (HOST; or both NULL) give every set's sorted support classes (concatenated; counts [sets], each <= c_task): the
 *   query rows are then filed under them as gm_meta_step does, and a class may have no rows.
 *   logits [subs, C], loss [sets], acc [sets]: always written.  dlogits [subs, C] (or NULL: no gradient): the loss's gradient, zero for subgraphs outside
 *   the class tables.  bwd != 0 (needs dlogits, dparams): dparams + t * dparam_stride receives dWl / dbl at wl_off / bl_off and nothing else; dQ [rows, Hd]
 *   receives relu'(H) * (dlogits @ Wl) at the centre rows -- NO other row is written, the call does no memset --, or Gc [subs * nc, Hd] the same rows in
 *   centre order (over either form of H): exactly one of the two with bwd, neither without.  sgd_next (or NULL; fused launch only): sgd_next_t = sgd_cur_t - sgd_lr * (dWl, dbl) at the same
 *   offsets, vectors sgd_stride apart.  dq_amax (or NULL; with dQ): uint32 slots t * 64, zeroed by the caller, receive the fp32 bits of max |dQ| written for set t.
 *   path 0: the fused k_head_loss; 1: k_head_fwd, k_proto, k_head_bwd as gm_gcn_forward / gm_proto_loss_* / gm_gcn_backward launch them (no SGD step).
 *   launched (HOST int32 [3], or NULL): {workgroup size, staged (LDS) 1 / 0, ragged instantiation 1 / 0} of the kernel that ran (path 1: 256, 0, k_proto's).
 * The call synchronises the stream.  GM_EINVAL: dQ together with Gc; mode 1 without protos; mode 0 with protos / dprotos; bwd without dlogits / dparams; an
 * output of the backward without bwd; the SGD step on path 1; dq_amax without dQ; nc that does not fit the batch; overlapping or too short strides; the
 * refusals of gm_proto_loss_*. */
int gm_dense_head_loss(const gm_batch_t* b, const float* H, int32_t Hd, int32_t nc, int32_t compact, int32_t C, const float* params,
                       int64_t param_stride, int64_t wl_off, int64_t bl_off, const int32_t* centre_local, const int32_t* y, int32_t mode,
                       int32_t n_support, const float* protos, int32_t c_task, const int32_t* spt_labels, const int32_t* spt_counts, float* logits,
                       float* dlogits, float* dprotos, float* protos_out, float* loss, float* acc, int32_t bwd, float* dparams,
                       int64_t dparam_stride, float* dQ, float* Gc, const float* sgd_cur, float* sgd_next, int64_t sgd_stride, float sgd_lr,
                       uint32_t* dq_amax, int32_t path, int32_t* launched, void* stream);

/* READOUT, gm_set_readout(mode): GM_READOUT_CENTRE (0, default: the head reads the centre row(s) of every subgraph, learner.py:159-170) or
 * GM_READOUT_MEAN (1: the alternative the reference left commented out, `#h = dgl.mean_nodes(g, 'h')`, learner.py:160); per calling thread, like
 * gm_set_ragged_classes and gm_set_hop_labels; any other value leaves the mode unchanged and sets gm_last_error.  Read at call time wherever a
 * gm_model_t is interpreted: gm_model_param_count, every *_ws_bytes, gm_meta_out_floats, gm_gcn_forward / _backward, gm_meta_step, gm_meta_adapt,
 * gm_proto_predict (call the size queries and the call they size under the same mode).  Under MEAN, per subgraph s with rows
 * [sub_off[s], sub_off[s+1]), n_s >= 1 of them, and H_L the (post-relu) output of the last GraphConv:
 *   forward   p_s = (sum_r H_L[r, :]) / n_s in fp32, in ONE fixed order that depends only on n_s and the model's width (rows in chunks of 64, a
 *             chunk's rows in a fixed strided order, the chunks of a subgraph in ascending order; no float atomics): two runs from the same state
 *             are bitwise identical;  logits_s = F.linear(p_s, W_lin, b_lin) with W_lin [n_out, dims[n_gcn]] -- for pair batches too: one pooled
 *             vector, no cat, so the parameter vector is n_out * dims[n_gcn] floats shorter than the pair model's under CENTRE;
 *   backward  dQ_L[r, :] = H_L[r, :] > 0 ? (dlogits_s W_lin) / n_s : 0 for EVERY row r of s;
 *   centre_local / the batch's centres are accepted and not used; pooling is topological and unweighted (edge weights and hop labels change H_L,
 *   not the pooling); ragged-task mode composes unchanged;
 *   schedules: hoist_z1 is honoured; sparse_bwd and cone are ignored (every row reaches the head: the dense schedule runs, same floats);
 *   gm_set_split_pieces(2) is ignored (three pieces, violation word 0).
 * With the mode off every call runs the kernels and launches it ran before the mode existed. */
#define GM_READOUT_CENTRE 0
#define GM_READOUT_MEAN 1
void gm_set_readout(int32_t mode);
int32_t gm_get_readout(void);

/* ---- The fused hot path: Meta.forward_ProtoMAML (meta.py:101-173) when need_meta_grad = 1,
 * Meta.finetunning_ProtoMAML (meta.py:175-234) when 0, for ALL sets (tasks) of spt/qry at once.
 * spt and qry must have the same number of sets; set t of each is task t.  y_spt / y_qry: HOST
 * int32 labels per subgraph.  theta: device fp32 [P] (read only).
 * out: device fp32 [P + 2*(K+1) + 1 + sets*(K+1) + 1] (= gm_meta_out_floats; out_floats is the capacity the caller allocated, checked):
 *   [0,P)            SUM over tasks of the first-order meta-gradient (query path at fw_K + prototype
 *                    path through the support forward at fw_{K-1}); zeros when need_meta_grad = 0
 *   [P, P+K+1)       SUM over tasks of losses_q[k]   (meta.py:133,140,155)
 *   [P+K+1, P+2K+2)  SUM over tasks of corrects[k]   (meta.py:134,141,157)
 *   [P+2K+2]         the number of tasks (sets) in this call, as a float (rides along with the all-reduce)
 *   [P+2K+3, ...)    per-task query accuracy [sets, K+1]
 *   [last]           violation word of the opt-in two-piece kernels as a float (0 = none; gm_set_split_pieces): when non-zero, losses_q[K]
 *                    above is NaN -- the step is skipped like a NaN loss on every rank -- and the caller re-runs it with three pieces
 * The caller divides by the (global) task count, applies the NaN guard (meta.py:163) and the
 * optimiser -- after the RCCL all-reduce when tasks are sharded over GPUs. */
int64_t gm_meta_ws_bytes(const gm_batch_t* spt, const gm_batch_t* qry, const gm_model_t* m, const gm_hparams_t* hp);
int64_t gm_meta_out_floats(const gm_batch_t* spt, const gm_model_t* m, const gm_hparams_t* hp);
int gm_meta_step(const gm_batch_t* spt, const gm_batch_t* qry, const int32_t* y_spt, const int32_t* y_qry,
                 const gm_model_t* m, const gm_hparams_t* hp, const float* theta, float* out, int64_t out_floats,
                 void* ws, int64_t ws_bytes, void* stream);

/* ---- Adaptation and prediction (beyond the reference, whose finetunning_ProtoMAML only scores labelled query sets).
 * gm_meta_adapt: the support chain of gm_meta_step alone, for every set (task) of spt: fw_0 = theta, fw_{k+1} = fw_k - update_lr * grad L_spt(fw_k)
 * for k < K = hp->update_step (K >= 0; hp->need_meta_grad must be 0; hoist_z1, sparse_bwd and cone are honoured; one stream).  y_spt: HOST int32
 * labels per subgraph; theta: device [P], 16-byte aligned.  fw_out: device [sets, fw_stride] (fw_stride >= P) <- fw_K in the caller's layout;
 * protos_out: device [sets, c_task, n_out] <- the prototypes of the support pass at fw_{max(K-1, 0)} -- the ones finetunning scores step K against
 * (meta.py:136-139,152-154) -- of set t's sorted classes, zero rows at and above its class count.  GM_EINVAL if c_task is below a set's class count.
 * gm_proto_predict: the query forward of every set s of qry at params + s * param_stride (caller's layout, param_stride >= P; gm_meta_step's
 * forward-only query pass), then per subgraph q of set s: a_qc = -|z_q - protos[s, c]|^2 over the first n_classes[s] (HOST int32 [sets], 1..c_task)
 * classes, logp_out[q, :] (device [subs, c_task]) = log_softmax(a_q), -inf at and above n_classes[s], pred_out[q] (device int32 [subs]) = its first
 * maximum (class 0 when all are NaN or equal); logits_out (device [subs, n_out] or NULL) <- z_q.  No labels: sets may have any size.
 * Both are stream-ordered (no host synchronisation) and always run the three-piece split kernels. */
int64_t gm_adapt_ws_bytes(const gm_batch_t* spt, const gm_model_t* m, const gm_hparams_t* hp);
int gm_meta_adapt(const gm_batch_t* spt, const int32_t* y_spt, const gm_model_t* m, const gm_hparams_t* hp, const float* theta, float* fw_out,
                  int64_t fw_stride, float* protos_out, int32_t c_task, void* ws, int64_t ws_bytes, void* stream);
int64_t gm_predict_ws_bytes(const gm_batch_t* qry, const gm_model_t* m, const gm_hparams_t* hp);
int gm_proto_predict(const gm_batch_t* qry, const gm_model_t* m, const gm_hparams_t* hp, const float* params, int64_t param_stride,
                     const float* protos, const int32_t* n_classes, int32_t c_task, float* logits_out, float* logp_out, int32_t* pred_out,
                     void* ws, int64_t ws_bytes, void* stream);

/* After the (optional) all-reduce of out[0 .. P + 2*(K+1)] over the ranks: the mean meta-gradient and the NaN guard of
 * meta.py:161-163, on the device.  head: device, the reduced block; grad: device fp32 [P] <- head[0..P) / task count;
 * found_inf: device fp32 [1] <- 1.0 if losses_q[K] / task count is NaN else 0.0 (a fused Adam skips its step on 1.0, which
 * is the reference's `if torch.isnan(loss_q): pass`).  K1 = update_step + 1. */
int gm_meta_finish(const float* head, int64_t P, int32_t K1, float* grad, float* found_inf, void* stream);
/* gm_meta_finish AND the Adam step of meta.py:97,161-169 (optim.Adam(lr = meta_lr): betas (0.9, 0.999), eps 1e-8, no weight decay) in one launch.
 * theta / exp_avg / exp_avg_sq: device fp32 [P], updated in place -- the parameters and the optimiser state torch.optim.Adam keeps (the host mirror
 * makes them views of flat buffers); steps: device fp32 [n_steps], the optimiser's per-parameter step counters (all equal), incremented together;
 * grad <- head[0..P) / task count as in gm_meta_finish; a NaN reduced query loss leaves theta, the state and the counters untouched and sets
 * found_inf = 1 (`if torch.isnan(loss_q): pass`).  ticket: device uint32 [1], zero before the first call (the kernel leaves it zero). */
int gm_meta_finish_adam(const float* head, int64_t P, int32_t K1, float* theta, float* exp_avg, float* exp_avg_sq, float* grad, float* steps, int32_t n_steps,
                        float lr, float beta1, float beta2, float eps, float* found_inf, uint32_t* ticket, void* stream);

/* Update-GEMM arithmetic (the reference multiplies in fp32: torch.matmul(feat, weight), learner.py:36,47).
 * mode 0: exact fp32 on v_mfma_f32_32x32x2_f32 everywhere.  mode 1 (default): large N = 128 / 256 launches run on the bf16 matrix cores
 * with every fp32 operand split EXACTLY into three bf16 pieces (8 + 8 + 8 significand bits: all 24 bits of both operands enter the
 * product) and the six products of weight >= 2^-16 accumulated in fp32 (dropped terms <= 1.2e-7 |a||b|: within one fp32 rounding per
 * product of the exact one; measured error against fp64 <= the fmaf chain's).  Also settable with GM_GEMM_MODE=f32|split.
 * gm_set_split_pieces(2) / GM_SPLIT_PIECES=2 is an OPT-IN fast mode, never the default: inside gm_meta_step (dense schedule,
 * aggregate-first layers) the split kernels then take TWO fp16 pieces per operand -- 22 significand bits, i.e. NARROWER than the
 * reference's fp32 operands -- with three products a_h b_h + a_h b_m + a_m b_h under per-task power-of-two scales derived from magnitude
 * bounds that the producing kernels record on the device (csrc/gm_bound.h).  Its guards: a feature table whose largest entry sits more
 * than 2^14 above its mean magnitude keeps the three-piece kernels for layer 1; a fast weight that outgrows the step's weight bound is
 * detected on the device and reported in the last float of gm_meta_step's `out` (the host mirror then re-runs the step three-piece).
 * gm_get_split_pieces() = 2 or 3. */
void gm_set_gemm_mode(int32_t mode);
int32_t gm_get_gemm_mode(void);
void gm_set_split_pieces(int32_t pieces);   /* 2, 3, or -1 = back to the environment variable (default 3) */
int32_t gm_get_split_pieces(void);
/* Tuning knob by the name of its environment variable, after start-up; GM_EINVAL for unknown names.  Tests use it to
 * force the large-launch kernels onto small fixtures (GM_GEMM_SPLIT_MIN_TILES, GM_SPLIT16_MIN_ROWS); not synchronised with concurrent calls. */
int gm_set_tuning(const char* name, int32_t value);
int32_t gm_get_tuning(const char* name);      /* current value of such a knob (0 for an unknown name) */
int32_t gm_tuning_epoch(void);   /* number of gm_set_tuning changes so far (cache key for sizes that depend on the knobs) */

/* Fused aggregate + update for forward passes nobody differentiates (the query evaluations of the inner steps in gm_meta_step,
 * i.e. meta.py:129-141,152-154 before the last step, and every query pass of finetunning): rows with one or two sources are
 * aggregated inside the GEMM's operand feeders, in the aggregate kernel's own fma order -- same floats, bit for bit -- and their
 * Z rows never travel through HBM.  on = 1 / 0, -1 = back to the environment variable GM_FUSE_AGG (default 1). */
void gm_set_fuse_agg(int32_t on);
int32_t gm_get_fuse_agg(void);

/* Profiling aid for bench.py: HIP-event time (ms) of the aggregate launches of the last
 * gm_meta_step on this thread, their count and their summed algorithmic bytes.  Events are only
 * recorded when gm_profile_enable(1) was called (they add a few microseconds per launch). */
void gm_profile_enable(int32_t on);
int gm_profile_aggregate(double* total_ms, int64_t* launches, int64_t* algorithmic_bytes);
/* Same for one launch category: 0 = aggregate (work = algorithmic bytes), 1 = grouped GEMM (forward and dZ; work =
 * flops 2*rows*K*N), 2 = weight gradient incl. its reduction (work = flops), 3 = the aggregate launches of category 0
 * priced at their COMPULSORY HBM bytes (a layer-1 launch that gathers from the store's feature table reads at most the
 * whole table, not rows*width; total_ms is 0 for this category -- use category 0's), 4 / 5 = the grouped GEMMs / weight
 * gradients that ran on the split-bf16 kernels (work = flops of the fp32 product; the kernels issue 6 bf16 MFMA flops per
 * fp32 flop) -- categories 1 / 2 then hold only the launches on the exact-fp32 MFMA kernels; 6 / 7 = the grouped GEMMs / weight
 * gradients on the two-piece fp16 split kernels (3 fp16 MFMA flops per fp32 flop).  Categories 8 / 9 / 10 belong to gm_extract on this thread
 * (not reset by gm_meta_step; gm_profile_enable resets them): 8 = k_nodes (h-hop expansion, sampling, node lists, induced degrees),
 * 9 = k_fill (the batched CSR in both orientations), work = subgraphs; 10 = batch finalisation (GPU span including its host round trips).
 * 12 = work-only: bytes by which the rounds-2/3 pricing of the partial aggregate launches (sources = min(edges, rows)) exceeds the exact count.
 * 11 = work-only shadow of categories 4 + 6: compulsory HBM bytes of the split GEMM launches, 4 rows (K + N) (A read once, C written once).
 * 13 / 14 = work-only: compulsory HBM bytes of EVERY grouped GEMM launch (A read once + the C rows stored) / of every weight-gradient launch
 * (A and G read once); 15 = the head + prototypical-loss launches (k_head_loss; work = subgraphs); 16 / 17 = the mean readout's forward
 * (k_readout_mean, k_readout_mean_fin) / backward (k_readout_mean_bwd) launches, work = algorithmic bytes 4 rows H + 4 subs H / 8 rows H + 4 subs H.  Under the receptive-field schedule
 * (gm_hparams_t.cone) category 0 is priced on the rows each level-to-level aggregate touches: destination-level row bounds and norms, the
 * edges between the two levels, every source-level row read once, every destination row written once. */
int gm_profile_read(int32_t category, double* total_ms, int64_t* launches, int64_t* work);
/* The same per launch: ms[k] / work[k] of the k-th timed launch of the category since the last reset (at most cap); returns their number (< 0: error). */
int gm_profile_read_launches(int32_t category, double* ms, int64_t* work, int32_t cap);
/* Timeline / phase probes used by tools/ (gm_debug_stamp, gm_stream_debug, gm_head_loss_debug) are NOT part of this library: they exist only in
 * the probe build, libgmeta_hip_probes.so (`python g-meta_amd/build.py --probes`), and are declared in include/gmeta_hip_probes.h. */

#ifdef __cplusplus
}
#endif
#endif /* GMETA_HIP_H */
