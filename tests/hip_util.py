"""GPU-side helpers shared by the -m gpu tests and __graft_entry__.smoke(): drive the HIP path
(through the Python host mirror, i.e. through the C ABI) on a golden fixture."""
import argparse
import random

import numpy as np
import torch

import gmeta_amd
from gmeta_amd import _lib
from gmeta_amd.subgraphs import SubgraphBatch


def make_store(fx):
    return gmeta_amd.GraphStore(fx.edges, fx.feats)


def fixture_batches(fx, store, replay):
    """Support / query mega-batches (one set per task) for a fixture."""
    out = {}
    for tag in ('spt', 'qry'):
        seeds = fx.z[tag + '_seeds']
        T, S = seeds.shape[:2]
        flat = seeds.reshape(-1, 3)
        off = np.arange(T + 1) * S
        if replay:
            lists = [fx.ref_nodes(tag, t, s) for t in range(T) for s in range(S)]
            out[tag] = SubgraphBatch.from_nodes(store, flat, off, lists, fx.link)
        else:
            out[tag] = SubgraphBatch.extract(store, flat, off, fx.args['h'], fx.args['sample_nodes'], 222, fx.link)
    return out['spt'], out['qry']


def fixture_meta(fx):
    args = argparse.Namespace(**fx.args)
    m = gmeta_amd.Meta(args, fx.config).to('cuda')
    with torch.no_grad():
        for p, v in zip(m.net.parameters(), fx.vars0):
            p.copy_(torch.from_numpy(v))
    return m


def hip_meta_step(fx, replay=True, hoist=0, sparse_bwd=0, cone=0, fused_adam_kernel=True):
    """Meta.forward on the fixture's meta-batch.  Returns accs, the meta-gradient that reached Adam,
    the updated weights and the node lists."""
    store = make_store(fx)
    S, Q = fixture_batches(fx, store, replay)
    m = fixture_meta(fx)
    m.hoist_z1 = hoist
    m.sparse_bwd = sparse_bwd
    m.cone = cone
    m.fused_adam_kernel = bool(fused_adam_kernel)
    ys = [torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_spt']]
    yq = [torch.from_numpy(y.astype(np.int64)) for y in fx.z['y_qry']]
    xs, xq = S.views(), Q.views()
    accs = m(xs, ys, xq, yq, None, None, None, None, None, None, fx.feats)
    # the meta-gradient that reached Adam = p.grad after the step (views of the flat buffer gm_meta_finish[_adam] wrote: the mean over the tasks)
    grad = torch.cat([p.grad.reshape(-1) for p in m.net.parameters()]).cpu().numpy().copy()
    res = {'accs': accs, 'grad': grad, 'vars1': [p.detach().cpu().numpy() for p in m.net.parameters()],
           'spt_parent': S.parent().astype(np.int64), 'qry_parent': Q.parent().astype(np.int64), 'stats': m.last_stats,
           'S': S, 'Q': Q, 'meta': m, 'store': store}
    return res


def arxiv_query_batch(T=8):
    """The query mega-batch of a synthetic arxiv meta-batch with T tasks (~286k rows at T = 8, one set per task) and its store: the
    full-size launch shape of the numerics tests of the GEMM and weight-gradient kernels."""
    from gmeta_amd import synth
    np.random.seed(222); random.seed(222); torch.manual_seed(222)
    args, cfg = synth.make_args('arxiv', task_num=T)
    data = synth.make_dataset(cfg)
    store = gmeta_amd.GraphStore(data['graphs'], data['feats'])
    db = gmeta_amd.Subgraphs(None, 'train', data['info'], n_way=3, k_shot=3, k_query=24, batchsz=T, args=args, adjs=store, h=2,
                             tables=data['tables'], verbose=False)
    batch = db.get_batch(list(range(T)))
    return batch[2][0].view_of, store


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def chunk_count(set_rows, n_cu):
    """Weight-gradient chunks of a batch with these set sizes: a restatement of gm_wgrad_chunk_rows (gm_internal.h)."""
    total, mx = sum(set_rows), max(1, max(set_rows))

    def chunks_at(cr):
        return sum((n + cr - 1) // cr for n in set_rows)
    best, best_eff = 128, -1.0
    for rounds in (1, 2, 3, 4, 6, 8):
        cap = n_cu * rounds
        lo, hi = 1, (mx + 31) // 32
        if chunks_at(32 * hi) > cap:
            continue
        while lo < hi:
            mid = (lo + hi) // 2
            if chunks_at(32 * mid) <= cap:
                hi = mid
            else:
                lo = mid + 1
        cr = max(128, 32 * lo)
        c = chunks_at(cr)
        eff = total / (((c + n_cu - 1) // n_cu) * n_cu * cr)
        if eff > best_eff + 0.25:
            best_eff, best = eff, cr
    return chunks_at(best)


class Batch:
    """A SubgraphBatch with what the numerics tests need: set row offsets, the batch's own norm (device pointer + a copy), its weight-gradient
    chunk count and GEMM tile count."""

    def __init__(self, B):
        self.B, self.T, self.rows = B, B.sets, B.rows
        self.so = [int(v) for v in B.sub_off[B.set_sub_off]]
        self.set_rows = [self.so[t + 1] - self.so[t] for t in range(self.T)]
        self.norm_ptr = B.device_ptr(_lib.F_NORM)
        self.norm = torch.from_numpy(B._read(_lib.F_NORM, B.rows, np.float32).copy()).cuda()
        self.n_chunks = chunk_count(self.set_rows, n_cus())
        self.n_tiles = sum((n + 127) // 128 for n in self.set_rows)          # GEMM row tiles of at most 128 rows, per set (gm_batch_finalize)


def synthetic_batch(set_rows, seed):
    """One subgraph per set with exactly set_rows[t] nodes of one random 1,100-node graph (SubgraphBatch.from_nodes)."""
    rng = np.random.default_rng(seed)
    n = 1100
    src, dst = rng.integers(0, n, 6 * n), rng.integers(0, n, 6 * n)
    store = gmeta_amd.GraphStore([(n, src.astype(np.int64), dst.astype(np.int64))], [rng.standard_normal((n, 8)).astype(np.float32)])
    lists = [np.sort(rng.choice(n, r, replace=False)).astype(np.int32) for r in set_rows]
    seeds = np.array([(0, int(l[0]), -1) for l in lists], np.int32)
    B = SubgraphBatch.from_nodes(store, seeds, np.arange(len(set_rows) + 1), lists, False)
    b = Batch(B)
    b.store = store
    assert b.set_rows == list(set_rows)
    return b
