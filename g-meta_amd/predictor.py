"""The BUDDY pair predictor on the hop-propagated features (gm_prop_pair_mlp_forward / gm_prop_pair_mlp_step; the definition is in include/gmeta_hip.h,
tests/pair_mlp_ref.py restates it): for a pair (a, b) of a graph with levels x_0 .. x_hops (PropagatedFeatures) and S caller-supplied structure columns s,

    z = [ op(x_0[a], x_0[b]) | ... | op(x_hops[a], x_hops[b]) | s ]      K = (hops + 1) feat_dim + S
    h = relu(z W1 + b1)                                                   W1 [K, hidden], in x out
    logit = h . w2 + b2,    loss = mean binary cross-entropy with logits

scored and differentiated on the device in fused kernels: the [m, K] matrix z never stands in memory, no gradient flows to the levels or to s (they are
precomputed, which is what makes BUDDY cheap).  Out of scope: dropout, batch norm, per-part linears (one hidden layer over the concatenation is their sum), and a
mask_target (the levels describe the whole graph)."""
import math

import numpy as np

from . import _lib
from .propagate import check_hops, check_op

MAX_HIDDEN = 256
MAX_EXTRA = 256


def pair_tile():
    """The pair tile T of the kernels: a workgroup scores T pairs (gm_prop_pair_mlp_tile)."""
    return int(_lib.lib().gm_prop_pair_mlp_tile())


class PairPredictor:
    """PairPredictor(feat_dim, hops, hidden=256, extra_dim=0, op='hadamard', seed=0): the weights of one predictor, not tied to a graph -- the same weights
    serve every graph's PropagatedFeatures of that feat_dim and hops.  `.params` is ONE flat torch.nn.Parameter on the device, [W1 row-major | b1 | w2 | b2];
    .W1 [K, hidden], .b1, .w2 [hidden], .b2 [1] are views of it.  Initialisation as torch.nn.Linear does it (Kaiming-uniform with a = sqrt(5): U(-1/sqrt(fan_in),
    1/sqrt(fan_in)) for a layer's weights and its bias), from a generator seeded with `seed`; the same generator shuffles the minibatches of .fit."""

    def __init__(self, feat_dim, hops, hidden=256, extra_dim=0, op='hadamard', seed=0):
        import torch
        self.op = op
        self.op_code = check_op(op, 'PairPredictor')
        self.hops = check_hops(hops, 'PairPredictor')
        self.feat_dim, self.hidden, self.extra_dim = int(feat_dim), int(hidden), int(extra_dim)
        if self.feat_dim < 1:
            raise ValueError('PairPredictor: feat_dim = %d' % self.feat_dim)
        if not 1 <= self.hidden <= MAX_HIDDEN:
            raise ValueError('PairPredictor: hidden = %d; 1 .. %d' % (self.hidden, MAX_HIDDEN))
        if not 0 <= self.extra_dim <= MAX_EXTRA:
            raise ValueError('PairPredictor: extra_dim = %d; 0 .. %d' % (self.extra_dim, MAX_EXTRA))
        self.K = (self.hops + 1) * self.feat_dim + self.extra_dim
        K, Hd = self.K, self.hidden
        self.generator = torch.Generator().manual_seed(int(seed))
        k1, k2 = 1.0 / math.sqrt(K), 1.0 / math.sqrt(Hd)
        draw = lambda n, k: (torch.rand(n, generator=self.generator, dtype=torch.float64) * 2.0 - 1.0) * k      # noqa: E731
        flat = torch.cat([draw(K * Hd, k1), draw(Hd, k1), draw(Hd, k2), draw(1, k2)]).to(torch.float32)
        self.params = torch.nn.Parameter(flat.cuda())

    # views of the flat parameter (they follow in-place updates of an optimiser)
    @property
    def W1(self):
        return self.params.data[:self.K * self.hidden].view(self.K, self.hidden)

    @property
    def b1(self):
        return self.params.data[self.K * self.hidden:self.K * self.hidden + self.hidden]

    @property
    def w2(self):
        return self.params.data[self.K * self.hidden + self.hidden:self.K * self.hidden + 2 * self.hidden]

    @property
    def b2(self):
        return self.params.data[-1:]

    def parameters(self):
        return [self.params]

    def _inputs(self, props, pairs, extra, what, sketches=None):
        """-> device int32 pairs [m, 2] (or None), device float32 structure columns [m, extra_dim] (or None), m.  With `sketches` the columns are
        [sketch columns | extra], built on the device: the sketch kernel writes into the [m, extra_dim] tensor with ld = extra_dim, extra is copied behind."""
        import torch
        if not getattr(props, 'handle', None):
            raise ValueError('%s: the propagated features are closed' % what)
        if props.feat_dim != self.feat_dim or props.hops != self.hops:
            raise ValueError('%s: propagated features of feat_dim = %d, hops = %d; the predictor has feat_dim = %d, hops = %d'
                             % (what, props.feat_dim, props.hops, self.feat_dim, self.hops))
        own = 0                                                                  # the columns the sketches fill
        if sketches is not None:
            if not getattr(sketches, 'handle', None):
                raise ValueError('%s: the sketches are closed' % what)
            if sketches.n_nodes != props.n_nodes:
                raise ValueError('%s: sketches of a graph with %d nodes; the propagated features have %d' % (what, sketches.n_nodes, props.n_nodes))
            own = sketches.n_columns
            given = 0 if extra is None else (int(extra.shape[1]) if getattr(extra, 'ndim', 0) == 2 else -1)
            if given < 0 or own + given != self.extra_dim:
                raise ValueError('%s: the sketches give %d columns and extra %s; the predictor has extra_dim = %d'
                                 % (what, own, 'none' if extra is None else 'shape %s' % (tuple(extra.shape),), self.extra_dim))
        width = self.extra_dim - own
        p = props._ids(pairs, what, (-1, 2))
        m = len(p)
        d_e = None
        if extra is None:
            if width:
                raise ValueError('%s: extra is None; the predictor has extra_dim = %d' % (what, self.extra_dim))
        elif isinstance(extra, torch.Tensor):
            if extra.dtype != torch.float32 or not extra.is_cuda:
                raise ValueError('%s: extra is a %s tensor on %s; a CUDA float32 tensor or a numpy array' % (what, extra.dtype, extra.device))
            if tuple(extra.shape) != (m, width):
                raise ValueError('%s: extra of shape %s; [%d, %d]' % (what, tuple(extra.shape), m, width))
            d_e = extra.contiguous()
        else:
            e = np.asarray(extra)
            if e.dtype not in (np.float32, np.float64):
                raise ValueError('%s: extra of dtype %s; float32 or float64' % (what, e.dtype))
            if e.shape != (m, width):
                raise ValueError('%s: extra of shape %s; [%d, %d]' % (what, e.shape, m, width))
            d_e = torch.from_numpy(np.ascontiguousarray(e, np.float32)).cuda()       # float64 is cast to float32 ONCE, here
        if width == 0:
            d_e = None
        d_p = torch.from_numpy(np.ascontiguousarray(p, np.int32)).cuda() if m else None
        if own:
            cols = torch.empty((m, self.extra_dim), dtype=torch.float32, device='cuda')
            if m:
                sketches._features_into(d_p, m, True, cols)
                if d_e is not None:
                    cols[:, own:] = d_e
            d_e = cols
        return d_p, d_e, m

    def scores(self, props, pairs, extra=None, as_torch=False, sketches=None):
        """float32 [m]: the logits of the [m, 2] node `pairs` of the graph of `props` (gm_prop_pair_mlp_forward).  A pair's logit is the same bits alone or in
        any batch, and for both of its orientations.  `extra`: the [m, extra_dim] structure columns, numpy (float64 is cast to float32 once) or a CUDA
        float32 tensor -- sketch_profile_features and distance_profile_features give them.  as_torch=True leaves the result on the device.
        `sketches`: the NodeSketches of the same graph; the structure columns are then [its pair_features (symmetric) | extra], built on the device with no
        read-back, and extra_dim must equal sketches.n_columns + the width of extra."""
        import torch
        d_p, d_e, m = self._inputs(props, pairs, extra, 'scores', sketches)
        out = torch.empty((m,), dtype=torch.float32, device='cuda')
        if m:
            _lib.check(_lib.lib().gm_prop_pair_mlp_forward(props.handle, _lib.ptr(d_p), m, self.op_code, _lib.ptr(d_e), self.extra_dim, _lib.ptr(self.params.data),
                                                           self.hidden, _lib.ptr(out), _lib.stream_ptr()), 'gm_prop_pair_mlp_forward')
        return out if as_torch else out.cpu().numpy()

    def step(self, props, pairs, labels, extra=None, sketches=None):
        """The mean binary cross-entropy of the logits against `labels` (numbers in [0, 1], or the tables' strings) as a float, and its gradient in
        .params.grad (OVERWRITTEN, as after zero_grad + backward) -- forward, loss and all gradients in one call (gm_prop_pair_mlp_step); any torch optimiser
        over .parameters() then steps.  `extra`, `sketches` as in .scores."""
        import torch
        d_p, d_e, m = self._inputs(props, pairs, extra, 'step', sketches)
        y = np.asarray(labels).reshape(-1).astype(np.float32)
        if len(y) != m:
            raise ValueError('step: %d labels, %d pairs' % (len(y), m))
        if m and not (np.isfinite(y).all() and y.min() >= 0.0 and y.max() <= 1.0):
            raise ValueError('step: a label outside [0, 1] (min %r, max %r)' % (float(np.nanmin(y)), float(np.nanmax(y))))
        d_y = torch.from_numpy(y).cuda() if m else None
        grad = torch.empty_like(self.params.data)
        loss = torch.empty((1,), dtype=torch.float32, device='cuda')
        _lib.check(_lib.lib().gm_prop_pair_mlp_step(props.handle, _lib.ptr(d_p), m, self.op_code, _lib.ptr(d_e), self.extra_dim, _lib.ptr(d_y), _lib.ptr(self.params.data),
                                                    self.hidden, None, _lib.ptr(loss), _lib.ptr(grad), _lib.stream_ptr()), 'gm_prop_pair_mlp_step')
        self.params.grad = grad
        return float(loss.item())

    @staticmethod
    def _names(names):
        from .heuristics import _pair
        return np.asarray([_pair(nm) for nm in names], np.int64).reshape(-1, 3)

    def link_scores(self, props_by_graph, names, extra=None, sketches=None, as_torch=False):
        """float32 [len(names)]: .scores of the pairs named 'g_i_j' from props_by_graph[g], one call per graph, rows in the order of `names`.  `sketches`: a dict or a
        sequence of NodeSketches by graph; the structure columns are then built on the device per call (.scores).  as_torch=True: the logits of every graph stay
        on the device and come back as one CUDA tensor (the same bits)."""
        trip = self._names(names)
        if as_torch:
            import torch
            out = torch.zeros(len(trip), dtype=torch.float32, device='cuda')
            for g in np.unique(trip[:, 0]).tolist():
                at = np.nonzero(trip[:, 0] == g)[0]
                out[torch.from_numpy(at).cuda()] = self.scores(props_by_graph[g], trip[at, 1:], None if extra is None else extra[at], as_torch=True,
                                                               sketches=None if sketches is None else sketches[g])
            return out
        out = np.zeros(len(trip), np.float32)
        for g in np.unique(trip[:, 0]).tolist():
            at = np.nonzero(trip[:, 0] == g)[0]
            out[at] = self.scores(props_by_graph[g], trip[at, 1:], None if extra is None else extra[at], sketches=None if sketches is None else sketches[g])
        return out

    def fit(self, props_by_graph, names, labels, extra=None, epochs=10, batch=4096, lr=0.01, sketches=None):
        """Trains with Adam on the pairs named 'g_i_j' (props_by_graph[g]: a dict or a sequence of PropagatedFeatures) and their 0 / 1 `labels`: per epoch the
        pairs of every graph, in ascending graph order, are shuffled by the predictor's seeded generator and walked in minibatches of `batch`, one .step per
        graph and minibatch -- the twin of link_propagated_features, without its [m, hops + 1, F] array.  `extra` (numpy [len(names), extra_dim]) rides along.
        `sketches` (a dict or a sequence of NodeSketches by graph): the sketch columns are built on the device per minibatch, in front of extra's, so that at most
        batch * extra_dim floats of them exist at a time and nothing per pair crosses to the host but the ids, the labels and the loss.
        -> the list of per-epoch losses (the mean of the minibatch losses, each weighted by its size)."""
        import torch
        trip = self._names(names)
        y = np.asarray(labels).reshape(-1).astype(np.float32)
        if len(y) != len(trip):
            raise ValueError('fit: %d labels, %d names' % (len(y), len(trip)))
        batch = int(batch)
        if batch < 1:
            raise ValueError('fit: batch = %d' % batch)
        if extra is not None:
            extra = np.asarray(extra)
        opt = torch.optim.Adam(self.parameters(), lr=lr)
        graphs = np.unique(trip[:, 0]).tolist()
        curve = []
        for _ in range(int(epochs)):
            total, seen = 0.0, 0
            for g in graphs:
                at = np.nonzero(trip[:, 0] == g)[0]
                at = at[torch.randperm(len(at), generator=self.generator).numpy()]
                for i in range(0, len(at), batch):
                    b = at[i:i + batch]
                    loss = self.step(props_by_graph[g], trip[b, 1:], y[b], None if extra is None else extra[b], sketches=None if sketches is None else sketches[g])
                    opt.step()
                    total += loss * len(b); seen += len(b)
            curve.append(total / max(seen, 1))
        return curve

    def auc(self, props_by_graph, names, labels, extra=None, sketches=None):
        """link_auc of .link_scores against the 0 / 1 `labels`."""
        from .heuristics import link_auc
        return link_auc(self.link_scores(props_by_graph, names, extra, sketches), labels)

    def ranking(self, props_by_graph, names, labels, ks=(20, 50, 100), extra=None, sketches=None, groups=None):
        """link_ranking (Hits@K, MRR, AUC from rank counts) of .link_scores against the 0 / 1 `labels`: the logits of every graph stay on the device,
        concatenated, and are ranked there -- nothing per pair is read back.  `groups` as in link_ranking."""
        from .ranking import link_ranking
        return link_ranking(self.link_scores(props_by_graph, names, extra, sketches, as_torch=True), labels, ks=ks, groups=groups)
