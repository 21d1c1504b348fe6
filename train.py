#!/usr/bin/env python3
"""train.py -- driver with the reference's flags and control flow (G-Meta/train.py:31-179) on the MI355X hot path.

    python train.py --data_dir DIR/ --task_setup Disjoint [--epoch 10 --task_num 32 --update_step 10 ...]

Differences from the reference driver, all at its edges: the graphs come from `graph_csr.npz` (see
g-meta_amd/datadir.py; DGL pickles cannot be read without DGL) and live in HBM as a GraphStore; a meta-batch is
extracted by two kernel launches (`Subgraphs.get_batch`) instead of a DataLoader over Python loops; validation/test
tasks are fine-tuned in ONE batched call.  With torch.distributed.run each rank takes a contiguous shard of every
meta-batch and the meta-gradient is all-reduced inside Meta.forward."""
import argparse
import copy
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import gmeta_amd                                   # noqa: E402
from gmeta_amd import datadir                      # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--epoch', type=int, default=10)
    ap.add_argument('--n_way', type=int, default=3)
    ap.add_argument('--k_spt', type=int, default=3)
    ap.add_argument('--k_qry', type=int, default=24)
    ap.add_argument('--task_num', type=int, default=8)
    ap.add_argument('--meta_lr', type=float, default=1e-3)
    ap.add_argument('--update_lr', type=float, default=1e-3)
    ap.add_argument('--update_step', type=int, default=5)
    ap.add_argument('--update_step_test', type=int, default=10)
    ap.add_argument('--input_dim', type=int, default=1)
    ap.add_argument('--hidden_dim', type=int, default=64)
    ap.add_argument('--attention_size', type=int, default=32)
    ap.add_argument('--data_dir', default=None, type=str, required=True)
    ap.add_argument('--no_finetune', default=True, type=str)
    ap.add_argument('--task_setup', default='Disjoint', type=str, required=True)
    ap.add_argument('--method', default='G-Meta', type=str)
    ap.add_argument('--task_n', type=int, default=1)
    ap.add_argument('--task_mode', default='False', type=str)
    ap.add_argument('--val_result_report_steps', default=100, type=int)
    ap.add_argument('--train_result_report_steps', default=30, type=int)
    ap.add_argument('--num_workers', default=0, type=int)
    ap.add_argument('--batchsz', default=1000, type=int)
    ap.add_argument('--link_pred_mode', default='False', type=str)
    ap.add_argument('--h', default=2, type=int)
    ap.add_argument('--sample_nodes', type=int, default=1000)
    ap.add_argument('--sample_mode', default='device', choices=['device', 'reference'],
                    help="'reference': draw oversize neighbourhoods exactly like the reference (global numpy RNG, CPython set order); slow, for reproducing its runs")
    ap.add_argument('--link_hops', default='reference', choices=['reference', 'symmetric'],
                    help="pair subgraphs (--link_pred_mode True): 'reference' = 2 hops around i and 1 hop around j whatever --h says, as the reference "
                         "builds them; 'symmetric' = --h hops around both endpoints")
    ap.add_argument('--hop_labels', type=int, default=0,
                    help='D in 1..7: append one-hot hop-distance labels (distance to the centre, to both endpoints of a pair; capped at D) to the '
                         'features of every subgraph; 0 = off')
    ap.add_argument('--mask_target', type=int, default=0, choices=[0, 1],
                    help='1 (--link_pred_mode True): build the subgraph of every pair without the edges between its two endpoints, as SEAL removes the target link; for '
                         'graphs that hold the positive pairs as edges and no injected negative ones')
    ap.add_argument('--negatives', default='file', choices=['file', 'uniform', 'two_hop'],
                    help="where the negative pairs of a link data set come from (--link_pred_mode True): 'file' = the CSV tables hold them, as the reference's do; "
                         "'uniform' / 'two_hop' = the tables hold the positive pairs only and as many negatives are drawn on the GPU from each graph's non-edges "
                         "(GraphStore.negative_pairs), the same on every rank; meant for --mask_target 1")
    ap.add_argument('--heuristics', type=int, default=0, choices=[0, 1, 2],
                    help='1 (--link_pred_mode True): after the test evaluation, print the ROC AUC of the five neighbourhood heuristics (common neighbours, Jaccard, '
                         'Adamic-Adar, resource allocation, preferential attachment; GraphStore.pair_scores) over the pairs of the test table -- the baseline a '
                         'learned link predictor is held against; follows --mask_target.  2: that line and a second one with the two path scores over walks of up to '
                         'three steps (local path index, truncated Katz index; GraphStore.pair_walks)')
    ap.add_argument('--pagerank', type=int, default=0, choices=[0, 1],
                    help='1 (--link_pred_mode True): after the test evaluation and the --heuristics lines, print the ROC AUC of the rooted PageRank score (the one global '
                         'baseline: GraphStore.pair_pagerank, alpha 0.15, 20 iterations) over the pairs of the test table; follows --mask_target, independent of --heuristics')
    ap.add_argument('--distance', type=int, default=0,
                    help='D in 1..254 (--link_pred_mode True): after the test evaluation and the --heuristics / --pagerank lines, print the ROC AUC of graph distance (the '
                         'shortest path of at most D edges, closer ranks higher: GraphStore.pair_distance) over the pairs of the test table; follows --mask_target, '
                         'independent of --heuristics and --pagerank; 0 = off')
    ap.add_argument('--buddy', type=int, default=0,
                    help='EPOCHS (--link_pred_mode True): after the test evaluation and the baseline lines, build the hop-propagated features (hops 2) and the '
                         'neighbourhood sketches of every graph, fit a BUDDY pair predictor (gmeta_amd.PairPredictor: level products + sketch profile columns) on the '
                         'pairs of the training table for EPOCHS epochs and print its ROC AUC over the pairs of the test table; 0 = off')
    ap.add_argument('--buddy_columns', default='host', choices=['host', 'device'],
                    help="where the sketch profile columns of --buddy are formed: 'host' = read the integers back and run the float64 estimators in numpy for every pair of "
                         "the train and test tables before the first step; 'device' = the predictor builds them per minibatch from the sketches "
                         "(NodeSketches.pair_features), nothing per pair is read back; needs --buddy > 0")
    ap.add_argument('--rank_k', default='',
                    help="K,K,... (up to 8 values, e.g. 20,50,100): after the ROC AUC line of every family the run scores (--heuristics, --pagerank, --distance, --buddy) "
                         "print one more line with its Hits@K and MRR over the pairs of the test table -- every positive against all negatives, all graphs "
                         "together, from rank counts formed on the device (gmeta_amd.link_ranking); '' = off")
    ap.add_argument('--holdout', type=int, default=0, choices=[0, 1],
                    help='1 (--link_pred_mode True, with --heuristics, --pagerank, --distance or --buddy): score those families on the graphs WITHOUT the positive pairs of '
                         'the validation and test tables (gmeta_amd.link_holdout: a store derived on the device), the protocol of the OGB link tasks -- no neighbourhood, '
                         'walk, distance, sketch or propagated feature sees a link that is being predicted; their lines end in "(held out)".  The meta-learning path '
                         'keeps the full graphs and --mask_target')
    ap.add_argument('--readout', default='centre', choices=['centre', 'mean'],
                    help="what the head reads of every subgraph: 'centre' = the centre row (both endpoints' rows of a pair), as the reference; 'mean' = the mean "
                         "over all of its rows (the dgl.mean_nodes line the reference left commented out), one pooled vector for pairs too")
    ap.add_argument('--eval_tasks', type=int, default=100, help='validation / test tasks (the reference hard-codes 100, train.py:90-91)')
    # schedules of the MI355X build that return the same results faster (include/gmeta_hip.h, gm_hparams_t); 0 = as the reference computes
    ap.add_argument('--hoist_z1', type=int, default=0, help='1: aggregate the layer-1 input once per meta-step instead of in every forward')
    ap.add_argument('--sparse_bwd', type=int, default=0, help='1: backward only over the rows whose gradient is structurally non-zero')
    ap.add_argument('--cone', type=int, default=0, help='1: evaluate each layer only on the rows that can reach a centre (forward and backward)')
    ap.add_argument('--ragged', type=int, default=0, choices=[0, 1],
                    help='1: tasks with short or imbalanced classes are trained and evaluated on (sample means over the rows that are there) instead of raising')
    ap.add_argument('--predict_out', default=None, type=str,
                    help='after the final test evaluation, label the query subgraphs of the test tasks with the early-stopped model and write them to this .npz')
    a = ap.parse_args(argv)
    if a.heuristics == 2 and a.link_pred_mode != 'True':      # refused before any data is read: node tasks have no pairs to score (--heuristics 1 keeps its check in main())
        raise SystemExit('--heuristics 2 scores node PAIRS: it needs --link_pred_mode True')
    if a.pagerank and a.link_pred_mode != 'True':
        raise SystemExit('--pagerank 1 scores node PAIRS: it needs --link_pred_mode True')
    if not 0 <= a.distance <= 254:
        raise SystemExit('--distance %d: 1 .. 254 (the longest path searched), 0 = off' % a.distance)
    if a.distance and a.link_pred_mode != 'True':
        raise SystemExit('--distance %d scores node PAIRS: it needs --link_pred_mode True' % a.distance)
    if a.buddy < 0:
        raise SystemExit('--buddy %d: epochs of the pair predictor, 0 = off' % a.buddy)
    if a.buddy and a.link_pred_mode != 'True':
        raise SystemExit('--buddy %d trains a predictor of node PAIRS: it needs --link_pred_mode True' % a.buddy)
    if a.buddy_columns != 'host' and not a.buddy:
        raise SystemExit('--buddy_columns %s chooses where the columns of the --buddy predictor are formed: it needs --buddy > 0' % a.buddy_columns)
    if a.holdout and a.link_pred_mode != 'True':
        raise SystemExit('--holdout 1 takes held-out node PAIRS out of the graphs: it needs --link_pred_mode True')
    if a.holdout and not (a.heuristics or a.pagerank or a.distance or a.buddy):
        raise SystemExit('--holdout 1 chooses the graphs a family is scored on: it needs --heuristics, --pagerank, --distance or --buddy')
    a.rank_ks = []
    if a.rank_k:
        try:
            a.rank_ks = [int(k) for k in a.rank_k.split(',')]
        except ValueError:
            raise SystemExit('--rank_k %s: comma-separated integers, e.g. 20,50,100' % a.rank_k)
        if not 1 <= len(a.rank_ks) <= 8 or min(a.rank_ks) < 1:
            raise SystemExit('--rank_k %s: one to eight values of K, each at least 1' % a.rank_k)
        if not (a.heuristics or a.pagerank or a.distance or a.buddy):
            raise SystemExit('--rank_k %s ranks the scores of a family: it needs --heuristics, --pagerank, --distance or --buddy' % a.rank_k)
    return a


def ranking_line(args, res, family, title, scores, labels, key='', tail=()):
    """--rank_k: res['<family>_ranking'] = {score name: gmeta_amd.link_ranking} of the family's scores over the test table, and the line behind its AUC line.
    --holdout: `key` behind the name in res, `tail` behind the line."""
    if not getattr(args, 'rank_ks', None):
        return
    family += '_ranking' + key
    res[family] = {nm: gmeta_amd.link_ranking(sc, labels, ks=args.rank_ks) for nm, sc in scores.items()}
    if int(os.environ.get('RANK', 0)) == 0:
        fmt = lambda m: ' '.join(['Hits@%d %.4f' % (k, m['hits@%d' % k]) for k in args.rank_ks] + ['MRR %.4f' % m['mrr']])      # noqa: E731
        one = len(scores) == 1
        print('%s test' % title, '  '.join(fmt(m) if one else '%s %s' % (nm, fmt(m)) for nm, m in res[family].items()), *tail)


def main(args):
    torch.manual_seed(222); np.random.seed(222); random.seed(222)          # train.py:33-35 (+ python RNG)
    rank = int(os.environ.get('RANK', 0)); world = int(os.environ.get('WORLD_SIZE', 1))
    if world > 1:
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)))
        torch.distributed.init_process_group('nccl')
    root = args.data_dir
    feat = datadir.load_features(root)
    graphs = datadir.load_graphs(root)
    if args.task_setup == 'Shared' and args.task_mode == 'True':            # train.py:49-51
        root = os.path.join(root, 'task' + str(args.task_n)) + '/'
    info = datadir.load_labels(root)
    store = gmeta_amd.GraphStore(graphs, feat)
    if args.heuristics and args.link_pred_mode != 'True':
        raise SystemExit('--heuristics %d scores node PAIRS: it needs --link_pred_mode True' % args.heuristics)
    tables = None
    if args.negatives != 'file':
        if args.link_pred_mode != 'True':
            raise SystemExit('--negatives %s draws negative PAIRS: it needs --link_pred_mode True' % args.negatives)
        from gmeta_amd.negatives import read_link_tables
        tables, info = gmeta_amd.link_tables_with_negatives(store, read_link_tables(root), info, mode=args.negatives)      # fixed seed: every rank draws the same pairs
        if rank == 0 and not args.mask_target:
            print('--negatives %s without --mask_target 1: the target edges of the positive pairs are visible to the model' % args.negatives)
    total_class = len(np.unique(np.array(list(info.values()))))
    labels_num = args.n_way if args.task_setup == 'Disjoint' else total_class   # train.py:58-61
    config = [('GraphConv', [feat[0].shape[1] + gmeta_amd.hop_label_width(args.hop_labels, args.link_pred_mode == 'True'), args.hidden_dim])]
    if args.h > 1:
        config = config + [('GraphConv', [args.hidden_dim, args.hidden_dim])] * (args.h - 1)
    config = config + [('Linear', [args.hidden_dim, labels_num])]
    if args.readout != 'centre':
        config.append(('Readout', [args.readout]))
    if args.link_pred_mode == 'True':
        config.append(('LinkPred', [True]))
    maml = gmeta_amd.Meta(args, config).to('cuda')
    if rank == 0:
        print('There are {} classes '.format(total_class))
        if store.weighted:
            print('The graphs carry edge weights (graph_csr.npz g*_w)')
        print('Total trainable tensors:', sum(int(np.prod(p.shape)) for p in maml.parameters() if p.requires_grad))
    mk = lambda mode, b: gmeta_amd.Subgraphs(root, mode, info, n_way=args.n_way, k_shot=args.k_spt, k_query=args.k_qry, batchsz=b,  # noqa: E731
                                             args=args, adjs=store, h=args.h, tables=tables, verbose=rank == 0)
    db_train, db_val, db_test = mk('train', args.batchsz), mk('val', args.eval_tasks), mk('test', args.eval_tasks)
    if world > args.task_num:
        raise SystemExit('task_num=%d cannot be sharded over %d ranks (every rank needs at least one task of a full meta-batch)' % (args.task_num, world))
    n_steps = -(-len(db_train) // args.task_num)      # DataLoader(db_train, task_num, shuffle=True) keeps the short last batch (drop_last=False, train.py:96)
    if n_steps == 0:
        raise SystemExit('batchsz=%d yields no meta-batch' % len(db_train))
    max_acc, model_max = 0, copy.deepcopy(maml)
    s_start = time.time()

    def evaluate(model, db):
        """train.py:115-123,129-141: fine-tune every val/test task.  Under torch.distributed the tasks are split over the ranks
        (independent, nothing is updated) and the accuracies all-gathered; every rank extracts only its slice."""
        n = len(db)
        if world > 1:
            b = np.linspace(0, n, world + 1).round().astype(int)
            mine = list(range(int(b[rank]), int(b[rank + 1])))
            x = db.get_batch(mine) if mine else ([], [], [], [])
            pad = lambda part: [None] * int(b[rank]) + list(part) + [None] * (n - int(b[rank + 1]))      # noqa: E731
            accs = model.finetunning_batch(pad(x[0]), pad(x[1]), pad(x[2]), pad(x[3]), shard=True)
        else:
            x = db.get_batch(list(range(n)))
            accs = model.finetunning_batch(x[0], x[1], x[2], x[3])
        return accs.mean(axis=0)                                                     # mean over tasks (train.py:123,136)

    for epoch in range(args.epoch):
        # DataLoader(shuffle=True) (train.py:96).  The permutation comes from a PRIVATE generator, identical on every rank: the
        # global numpy RNG belongs to the node sampler of --sample_mode reference (sdp.py:313), whose consumption differs per rank.
        order = np.random.RandomState(222 + epoch).permutation(len(db_train))
        shards = []
        for step in range(n_steps):
            chunk = order[step * args.task_num:(step + 1) * args.task_num]            # the last one may be short
            b = np.linspace(0, len(chunk), world + 1).round().astype(int)
            shards.append(chunk[int(b[rank]):int(b[rank + 1])])                       # may be empty on a short trailing batch: contributes zeros
        # num_workers (train.py:96,173): depth of the look-ahead -- meta-batches built ahead by ONE builder thread on its own stream.  (Subgraphs.batches(workers=N) keeps
        # N builds in flight; measured in round 6 it only helps while a build is host-latency-bound -- since the joint build of both batches it is GPU-bound and a
        # second builder's kernels slow a short meta-step down more than they hide: profiles/r06_experiments_not_shipped.txt F)
        it = iter(db_train.batches(shards, prefetch=args.num_workers, cone_layers=args.h if getattr(args, 'cone', 0) else 0,
                                   workers=1))
        for step in range(n_steps):
            s = time.time()
            batch = next(it)            # extracted by the prefetch thread while the previous meta-step ran (num_workers > 0)
            t_load = time.time() - s
            s = time.time()
            report = step % args.train_result_report_steps == 0
            res = maml.forward_deferred(*batch[:4])      # whole meta-step incl. all-reduce + Adam queued on the GPU
            if report:                                   # the accuracies are only read when they are printed (train.py:110)
                accs = res.accs()
                if rank == 0:
                    print('Epoch:', epoch + 1, ' Step:', step, ' training acc:', str(accs[-1])[:5], ' time elapsed:', str(time.time() - s)[:5],
                          ' data loading takes:', str(t_load)[:5])
        accs = evaluate(maml, db_val)
        if rank == 0:
            print('Epoch:', epoch + 1, ' Val acc:', str(accs[-1])[:5])
        if accs[-1] > max_acc:
            max_acc, model_max = accs[-1], copy.deepcopy(maml)                       # train.py:125-127
    accs = evaluate(maml, db_test)
    accs_max = evaluate(model_max, db_test)
    if rank == 0:
        print('Test acc:', str(accs[-1])[:5])
        print('Early Stopped Test acc:', str(accs_max[-1])[:5])
        print('Total Time:', str(time.time() - s_start)[:5])
    if args.predict_out and rank == 0:
        write_predictions(args.predict_out, model_max, db_test, info)
    res = {'test_acc': float(accs[-1]), 'early_stopped_test_acc': float(accs_max[-1]), 'val_best': float(max_acc)}
    full, key, tail = store, '', ()
    if getattr(args, 'holdout', 0):
        # the families below score the test pairs in the graphs without the validation and test positives; Subgraphs / Meta above kept the full store
        from gmeta_amd.negatives import read_link_tables
        store, key, tail = gmeta_amd.link_holdout(full, tables if tables is not None else read_link_tables(root)), '_holdout', ('(held out)',)
    try:
        family_lines(args, res, store, tables, root, rank, key, tail)
    finally:
        if store is not full:
            store.close()
    return res


def family_lines(args, res, store, tables, root, rank, key, tail):
    """The baseline families of --heuristics / --pagerank / --distance / --buddy over the test table, scored on `store`: their entries of `res` (names end in
    `key`) and their lines (end in `tail`)."""
    if args.heuristics:
        # the test table as the run used it: completed by --negatives where that drew the negative pairs, else the CSV's own
        from gmeta_amd.negatives import read_link_tables
        names, labels = (tables if tables is not None else read_link_tables(root))['test']
        res['heuristic_auc' + key] = gmeta_amd.link_heuristic_auc(store, names, labels, mask_target=bool(args.mask_target))
        if rank == 0:
            print('Heuristic test AUC:', '  '.join('%s %.4f' % (k, v) for k, v in res['heuristic_auc' + key].items()), *tail)
        if getattr(args, 'rank_ks', None):
            from gmeta_amd.heuristics import link_heuristic_scores
            sc = link_heuristic_scores(store, names, bool(args.mask_target))
            ranking_line(args, res, 'heuristic', 'Heuristic', {nm: sc[:, k] for k, nm in enumerate(gmeta_amd.PAIR_SCORES)}, labels, key, tail)
        if args.heuristics == 2:
            res['path_auc' + key] = gmeta_amd.link_path_auc(store, names, labels, mask_target=bool(args.mask_target))
            if rank == 0:
                print('Path test AUC:', '  '.join('%s %.4f' % (k, v) for k, v in res['path_auc' + key].items()), *tail)
            if getattr(args, 'rank_ks', None):
                w = gmeta_amd.link_path_scores(store, names, bool(args.mask_target))
                ranking_line(args, res, 'path', 'Path', {'local_path': gmeta_amd.local_path_index(w), 'katz': gmeta_amd.katz_index(w)}, labels, key, tail)
    if args.pagerank:
        from gmeta_amd.negatives import read_link_tables
        names, labels = (tables if tables is not None else read_link_tables(root))['test']
        res['pagerank_auc' + key] = gmeta_amd.link_pagerank_auc(store, names, labels, mask_target=bool(args.mask_target))
        if rank == 0:
            print('PageRank test AUC:', '  '.join('%s %.4f' % (k, v) for k, v in res['pagerank_auc' + key].items()), *tail)
        if getattr(args, 'rank_ks', None):
            cols = gmeta_amd.link_pagerank_scores(store, names, bool(args.mask_target))
            ranking_line(args, res, 'pagerank', 'PageRank', {'rooted_pagerank': gmeta_amd.rooted_pagerank_index(cols)}, labels, key, tail)
    if args.distance:
        from gmeta_amd.negatives import read_link_tables
        names, labels = (tables if tables is not None else read_link_tables(root))['test']
        res['distance_auc' + key] = gmeta_amd.link_distance_auc(store, names, labels, mask_target=bool(args.mask_target), max_dist=args.distance)
        if rank == 0:
            print('Distance test AUC:', '  '.join('%s %.4f' % (k, v) for k, v in res['distance_auc' + key].items()), *tail)
        if getattr(args, 'rank_ks', None):
            d = gmeta_amd.link_distance_scores(store, names, bool(args.mask_target), args.distance)
            ranking_line(args, res, 'distance', 'Distance', {'graph_distance': gmeta_amd.graph_distance_index(d, args.distance)}, labels, key, tail)
    if args.buddy:
        from gmeta_amd.negatives import read_link_tables
        both = tables if tables is not None else read_link_tables(root)
        logits = [] if getattr(args, 'rank_ks', None) else None
        res['buddy_auc' + key] = buddy_auc(store, both['train'], both['test'], args.buddy, columns=args.buddy_columns, logits=logits)
        if rank == 0:
            print('BUDDY test AUC: %.4f' % res['buddy_auc' + key], *tail)
        if getattr(args, 'rank_ks', None):
            ranking_line(args, res, 'buddy', 'BUDDY', {'buddy': logits[0]}, both['test'][1], key, tail)      # the fitted predictor's logits, still on the device


def buddy_auc(store, train, test, epochs, hops=2, columns='host', logits=None):
    """The two precomputed inputs of a BUDDY predictor for every graph (the levels of GraphStore.propagated_features and the sketches of GraphStore.sketches, both
    at `hops`), a gmeta_amd.PairPredictor fitted on the (names, labels) of `train`, and its ROC AUC over those of `test`.  No mask_target: both inputs describe the
    whole graph of `store` -- pass gmeta_amd.link_holdout(store, tables) (train.py --holdout 1) so that neither holds a pair of `test` as an edge.  columns='host': the sketch profile columns of every pair of both tables are formed up front by the float64 host estimators;
    'device': the predictor forms them per minibatch on the device from the sketches (PairPredictor.fit / .auc with sketches=).  `logits`: a list that
    receives the fitted predictor's logits of `test` as one CUDA tensor (PairPredictor.link_scores(..., as_torch=True)), for --rank_k."""
    graphs = range(store.n_graphs)
    props = [store.propagated_features(g, hops=hops) for g in graphs]
    sketches = [store.sketches(g, hops=hops) for g in graphs]
    try:
        if columns == 'device':
            model = gmeta_amd.PairPredictor(store.feat_dim, hops, extra_dim=(hops + 2) ** 2, seed=222)
            model.fit(props, train[0], train[1], epochs=epochs, sketches=sketches)
            if logits is not None:
                logits.append(model.link_scores(props, test[0], sketches=sketches, as_torch=True))
            return model.auc(props, test[0], test[1], sketches=sketches)
        columns = lambda names: gmeta_amd.sketch_profile_features(gmeta_amd.link_sketch_profiles(sketches, names))      # noqa: E731
        x_train, x_test = columns(train[0]), columns(test[0])
        model = gmeta_amd.PairPredictor(store.feat_dim, hops, extra_dim=x_train.shape[1], seed=222)
        model.fit(props, train[0], train[1], extra=x_train, epochs=epochs)
        if logits is not None:
            logits.append(model.link_scores(props, test[0], extra=x_test, as_torch=True))
        return model.auc(props, test[0], test[1], extra=x_test)
    finally:
        for o in props + sketches:
            o.close()


def write_predictions(path, model, db, info):
    """Meta.predict on every task of `db` (same tasks and K_test as the final evaluation).  The .npz holds, flattened over the tasks with
    per-task offsets `task_off`: `names` (query subgraph names), `true` / `pred` (label values of the dataset's label.pkl) and `log_probs`
    [n, c_max] (column c of task t = label value classes[class_off[t] + c]; -inf past the task's class count)."""
    tasks = list(range(len(db)))
    x = db.get_batch(tasks)
    pr = model.predict(x[0], x[1], x[2])
    names, true, pred, logp, classes, off, coff = [], [], [], [], [], [0], [0]
    c_max = max(lp.shape[1] for lp in pr.log_probs)
    for t in tasks:
        spt_names, qry_names = db._task_names(t)
        raw = {int(r): info[n] for r, n in zip(np.asarray(x[1][t]).reshape(-1), spt_names)}      # per-task rank (Disjoint relabelling) -> label value
        names += qry_names
        true += [info[n] for n in qry_names]
        pred += [raw[int(c)] for c in pr.labels[t]]
        lp = np.full((len(qry_names), c_max), -np.inf, np.float32)
        lp[:, :pr.log_probs[t].shape[1]] = pr.log_probs[t]
        logp.append(lp)
        classes += [raw[int(c)] for c in pr.classes[t]]
        off.append(len(names)); coff.append(len(classes))
    np.savez(path, names=np.asarray(names), true=np.asarray(true), pred=np.asarray(pred), log_probs=np.concatenate(logp),
             classes=np.asarray(classes), task_off=np.asarray(off, np.int64), class_off=np.asarray(coff, np.int64))


if __name__ == '__main__':
    main(parse())
