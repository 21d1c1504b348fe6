"""Host side of Meta.adapt / Meta.predict: without a GPU they fail like every other entry point (no CPU fallback)."""
import argparse

import numpy as np
import pytest
import torch


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_adapt_and_predict_fail_loudly_without_gpu():
    import gmeta_amd
    args = argparse.Namespace(update_lr=0.01, meta_lr=1e-3, n_way=2, k_spt=1, k_qry=2, task_num=1, update_step=2, update_step_test=3,
                              method='G-Meta')
    m = gmeta_amd.Meta(args, [('GraphConv', [4, 8]), ('Linear', [8, 2])])
    y = [np.array([0, 1])]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.adapt([None], y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.predict([None], y, [None])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.adapt([None], y, K=-1)


def test_prediction_api_is_exported():
    from gmeta_amd import _lib
    from gmeta_amd.meta import Adapted, Meta, Prediction
    assert callable(Meta.adapt) and callable(Meta.predict) and callable(Adapted.predict) and Prediction is not None
    for name in ('gm_adapt_ws_bytes', 'gm_meta_adapt', 'gm_predict_ws_bytes', 'gm_proto_predict'):
        assert name in _lib.PROTOTYPES
