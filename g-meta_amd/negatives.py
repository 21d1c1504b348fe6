"""Negative pairs for link-prediction tables.  A user's own graph holds the positive pairs as edges and no injected negative ones (with
Subgraphs(mask_target=True)); `link_tables_with_negatives` completes positives-only tables with pairs drawn by GraphStore.negative_pairs
(gm_store_negative_pairs; the definition is in include/gmeta_hip.h)."""
import numpy as np

SPLITS = ('train', 'val', 'test')
PARTS = ('_spt', '_qry')


def read_link_tables(root):
    """The {train,val,test}{,_spt,_qry}.csv files of a data directory that exist, as the `tables=` dictionary of Subgraphs: name -> (names, labels)."""
    import csv
    import os
    tables = {}
    for split in SPLITS:
        for part in ('',) + PARTS:
            p = os.path.join(root, split + part + '.csv')
            if not os.path.exists(p):
                continue
            names, labels = [], []
            with open(p) as f:
                rd = csv.reader(f, delimiter=',')
                next(rd, None)
                for row in rd:
                    names.append(row[1]); labels.append(row[2])
            tables[split + part] = (names, labels)
    return tables


def _pair(name):
    f = name.split('_')
    if len(f) != 3:
        raise ValueError("link tables hold names 'g_i_j'; got %r" % (name,))
    return int(f[0]), int(f[1]), int(f[2])


def link_tables_with_negatives(store, tables, info, mode='uniform', seed=222):
    """Positives-only link tables -> (tables, info) completed with as many negatives.

    `tables` is a `tables=` dictionary of Subgraphs: keys {train,val,test} x {'', '_spt', '_qry'} (absent ones are skipped), names 'g_i_j', every label
    '1' (ValueError otherwise).  Per graph, ONE store.negative_pairs(g, total, seed, mode, exclude=...) call draws `total` = the graph's positives over
    the six _spt / _qry tables; `exclude` is every positive pair any table lists for the graph, so a positive that was taken out of the graph for
    validation or test cannot come back as a negative.  The pairs are dealt out in order to train_spt, train_qry, val_spt, val_qry, test_spt, test_qry, as
    many as each holds positives of the graph, named 'g_u_v' and labelled '0', behind the table's positives; every plain split table becomes the
    concatenation of its two parts.  `info` gains the new names with the int label 0.  Neither input is modified."""
    for key, (names, labels) in tables.items():
        bad = sorted({str(l) for l in labels} - {'1'})
        if bad:
            raise ValueError("link_tables_with_negatives takes positives-only tables: table %r already holds label(s) %s" % (key, ', '.join(bad)))
        if len(names) != len(labels):
            raise ValueError('table %r: %d names, %d labels' % (key, len(names), len(labels)))
    part_keys = [s + p for s in SPLITS for p in PARTS if s + p in tables]
    per_graph, exclude = {}, {}                         # g -> {part key: positives}, g -> every positive pair listed anywhere
    for key, (names, _) in tables.items():
        for nm in names:
            g, i, j = _pair(nm)
            exclude.setdefault(g, []).append((i, j))
            if key in part_keys:
                cnt = per_graph.setdefault(g, {})
                cnt[key] = cnt.get(key, 0) + 1
    out = {key: (list(names), [str(l) for l in labels]) for key, (names, labels) in tables.items()}
    info = dict(info)
    for g in sorted(per_graph):
        total = sum(per_graph[g].values())
        neg = np.asarray(store.negative_pairs(g, total, seed=seed, mode=mode, exclude=np.asarray(exclude[g], np.int64).reshape(-1, 2))).reshape(-1, 2)
        if len(neg) != total:
            raise ValueError('negative_pairs returned %d pairs for graph %d, %d asked for' % (len(neg), g, total))
        at = 0
        for key in part_keys:
            for u, v in neg[at:at + per_graph[g].get(key, 0)].tolist():
                nm = '%d_%d_%d' % (g, u, v)
                out[key][0].append(nm); out[key][1].append('0')
                info[nm] = 0
            at += per_graph[g].get(key, 0)
    for s in SPLITS:
        if s in out:
            parts = [out[s + p] for p in PARTS if s + p in out]
            if parts:
                out[s] = ([nm for names, _ in parts for nm in names], [l for _, labels in parts for l in labels])
    return out, info


def link_holdout(store, tables, splits=('val', 'test')):
    """The store without the positive pairs of the named `splits`: from a `tables=` dictionary (read_link_tables / link_tables_with_negatives: key ->
    (names 'g_i_j', labels)) the pairs labelled 1 in each split's plain table -- or, where that is absent, in its _spt / _qry parts -- are collected per graph
    and taken out with store.without_edges (gm_store_without_edges).  Score the validation and test pairs on the result: no structural input computed from
    it -- neighbourhoods, walks, distances, sketches, propagated features -- holds a link that is being predicted.  Negative pairs name no edge and are
    skipped.  The caller closes the returned store."""
    removed = {}
    for s in splits:
        if s not in SPLITS:
            raise ValueError('link_holdout: split %r; one of %s' % (s, ', '.join(SPLITS)))
        keys = [s] if s in tables else [s + p for p in PARTS if s + p in tables]
        for key in keys:
            names, labels = tables[key]
            for nm, lab in zip(names, labels):
                if int(lab) == 1:
                    g, i, j = _pair(nm)
                    removed.setdefault(g, []).append((i, j))
    return store.without_edges({g: np.asarray(p, np.int64).reshape(-1, 2) for g, p in removed.items()})
