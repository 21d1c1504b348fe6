"""On-disk adapter for G-Meta data directories.

The reference loads (train.py:41-53): `features.npy` (2-D array, or object array of per-graph matrices),
`graph_dgl.pkl` (pickled list of dgl.DGLGraph 0.4.3 objects -- NOT readable without DGL), `label.pkl`
(dict name -> label) and `{train,val,test}.csv` (+ `_spt` / `_qry` variants for link prediction).
This build reads the same files except the DGL pickle, which is replaced by `graph_csr.npz`:
    n_graphs, and per graph g:  g{g}_n, g{g}_src, g{g}_dst   (directed edge list, edge k: src -> dst)
    and optionally g{g}_w (fp32, one weight per edge; beyond the reference): the graphs then load as (n, src, dst, w) and GraphStore builds a weighted store
`convert_dgl_pickle` produces it wherever DGL is importable; `write_datadir` writes a complete directory
(used by the synthetic generators and the tests)."""
import os
import pickle

import numpy as np


def load_features(root):
    feat = np.load(os.path.join(root, 'features.npy'), allow_pickle=True)
    if feat.dtype != object and feat.ndim == 2:          # single graph (train.py:63-65)
        return [np.ascontiguousarray(feat, np.float32)]
    return [np.ascontiguousarray(f, np.float32) for f in feat]


def load_graphs(root):
    p = os.path.join(root, 'graph_csr.npz')
    if os.path.exists(p):
        z = np.load(p)
        return [(int(z['g%d_n' % g]), z['g%d_src' % g], z['g%d_dst' % g]) + ((z['g%d_w' % g],) if 'g%d_w' % g in z.files else ())
                for g in range(int(z['n_graphs']))]
    pk = os.path.join(root, 'graph_dgl.pkl')
    if os.path.exists(pk):
        try:
            import dgl  # noqa: F401
        except ImportError:
            raise RuntimeError('%s is a pickle of DGL 0.4.3 graphs and DGL is not installed here; run '
                               'gmeta_amd.datadir.convert_dgl_pickle(root) where DGL is available to write graph_csr.npz' % pk)
        return convert_dgl_pickle(root)
    raise FileNotFoundError('neither graph_csr.npz nor graph_dgl.pkl in %s' % root)


def convert_dgl_pickle(root):
    """Run where dgl is importable: graph_dgl.pkl -> graph_csr.npz (edge lists in DGL edge-id order)."""
    with open(os.path.join(root, 'graph_dgl.pkl'), 'rb') as f:
        gs = pickle.load(f)
    graphs = []
    for g in gs:
        u, v = g.edges()
        graphs.append((int(g.number_of_nodes()), np.asarray(u), np.asarray(v)))
    save_graphs(root, graphs)
    return graphs


def save_graphs(root, graphs):
    out = {'n_graphs': len(graphs)}
    for g, gr in enumerate(graphs):
        n, src, dst = gr[:3]
        out['g%d_n' % g] = n
        out['g%d_src' % g] = np.asarray(src, np.int32)
        out['g%d_dst' % g] = np.asarray(dst, np.int32)
        if len(gr) == 4:                                   # optional edge weights
            out['g%d_w' % g] = np.asarray(gr[3], np.float32)
    np.savez(os.path.join(root, 'graph_csr.npz'), **out)


def load_labels(root):
    with open(os.path.join(root, 'label.pkl'), 'rb') as f:
        return pickle.load(f)


def write_csv(path, names, labels):
    """Same 3-column layout pandas' DataFrame({'name','label'}).to_csv gives (sdp.py:126-130 skips the header, reads cols 1,2)."""
    with open(path, 'w') as f:
        f.write(',name,label\n')
        for k, (a, b) in enumerate(zip(names, labels)):
            f.write('%d,%s,%s\n' % (k, a, b))


def write_datadir(root, graphs, feats, info, splits):
    """splits: {'train': (names, labels), 'val': ..., 'test': ...} (plus '*_spt' / '*_qry' for link prediction)."""
    os.makedirs(root, exist_ok=True)
    save_graphs(root, graphs)
    if len(feats) == 1:
        np.save(os.path.join(root, 'features.npy'), np.asarray(feats[0], np.float32))
    else:
        arr = np.empty(len(feats), dtype=object)
        for k, f in enumerate(feats):
            arr[k] = np.asarray(f, np.float32)
        np.save(os.path.join(root, 'features.npy'), arr, allow_pickle=True)
    with open(os.path.join(root, 'label.pkl'), 'wb') as f:
        pickle.dump(dict(info), f)
    for name, (names, labels) in splits.items():
        write_csv(os.path.join(root, name + '.csv'), names, labels)
