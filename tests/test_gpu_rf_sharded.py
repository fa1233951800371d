"""Row-sharded forest training on the GPU: dal.parallel.emulate_train_* (P
jobs through the level-step HIP entries, the all-reduce as an elementwise
sum) and dal.parallel.train_* on a one-rank RCCL group (the real all-reduce
on the workspace span) against dal.random_forest.train_classifier /
train_regressor of the same rows in position order on the same device, byte
for byte.

Shapes: 600 x 8 with features quantised to 12 values (bins tie) and noisy
labels; 600 x 5 regression with y = 1e6 + noise 1e-3 (two limbs of y); and
12,000 x 3 -- above the 10,000 rows at which the split sample is drawn --
in shards of 1,100 / 5,000 / 5,900 rows, each more than the statistics
kernel's 1,024 rows per block, so the sample spans every shard."""
import os
import socket

import numpy as np
import pytest

from rf_sharded_reference import contiguous as _contiguous
from rf_sharded_reference import interleaved as _interleaved

pytestmark = pytest.mark.gpu

N, D, T, DEPTH = 600, 8, 5, 4
RN, RD, RT = 600, 5, 6
BN, BD, BT, BDEPTH = 12000, 3, 2, 3


def _class_pool(C, n=N, d=D, seed=21):
    rng = np.random.default_rng(seed)
    X = (np.floor(rng.random((n, d)) * 12) / 4).astype(np.float32)
    y = ((X[:, 0] * 4 + X[:, 1] * 2 + rng.random(n) * 6).astype(np.int64) // 3) % C  # noisy
    return X, y


def _reg_pool(f64, n=RN, d=RD, seed=22):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    y = 1e6 + (X[:, 0] - X[:, 1] + rng.standard_normal(n)) * 1e-3
    return (X if f64 else X.astype(np.float32)), y


def _shards(X, y, parts):
    return [(X[p], y[p], p) for p in parts]


def _thresholds(model):
    thr, ns = (t.cpu().numpy() for t in model.split_thresholds)
    return [thr[f, :ns[f]].tobytes() for f in range(thr.shape[0])]


def _bytes(model):
    names = ("inner_feature", "inner_threshold", "leaf") if hasattr(model, "inner_feature") else ("inner", "leaf")
    return [getattr(model, a).tobytes() for a in names] + _thresholds(model)


_SINGLE = {}


def _single(key):
    """The single-device fits, each computed once."""
    from dal import random_forest as rf

    if key not in _SINGLE:
        kind, arg = key
        if kind == "class":
            X, y = _class_pool(arg)
            _SINGLE[key] = rf.train_classifier(X, y, num_trees=T, max_depth=DEPTH, seed=3, num_classes=arg)
        elif kind == "reg":
            X, y = _reg_pool(arg)
            _SINGLE[key] = rf.train_regressor(X, y, num_trees=RT, max_depth=DEPTH, seed=4)
        elif kind == "big_class":
            X, y = _class_pool(2, BN, BD, seed=23)
            _SINGLE[key] = rf.train_classifier(X, y, num_trees=BT, max_depth=BDEPTH, seed=5)
        else:
            X, y = _reg_pool(False, BN, BD, seed=24)
            _SINGLE[key] = rf.train_regressor(X, y, num_trees=BT, max_depth=BDEPTH, seed=6)
    return _SINGLE[key]


def _fit_class(C, parts):
    from dal import parallel

    X, y = _class_pool(C)
    return parallel.emulate_train_classifier(_shards(X, y, parts), N, num_trees=T, max_depth=DEPTH, seed=3,
                                             num_classes=C)


@pytest.mark.parametrize("scheme", ["one", "contiguous", "interleaved_empty"])
def test_binary_shards_equal_the_single_device_fit(cuda, scheme):
    parts = {"one": [np.arange(N)], "contiguous": _contiguous(N, [1, 250, 349]),
             "interleaved_empty": _interleaved(N, 4, empty=2)}[scheme]
    assert _bytes(_fit_class(2, parts)) == _bytes(_single(("class", 2)))


@pytest.mark.parametrize("C", [3, 5])
def test_multiclass_shards_equal_the_single_device_fit(cuda, C):
    assert _bytes(_fit_class(C, _interleaved(N, 3))) == _bytes(_single(("class", C)))


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("P,chunk", [(3, None), (2, 1), (2, 4), (2, None)])
def test_regressor_shards_equal_the_single_device_fit(cuda, f64, P, chunk):
    from dal import parallel
    from dal import random_forest as rf

    X, y = _reg_pool(f64)
    assert rf.check_regression_labels(y, RN)[1][1] >= 2  # k_y: more than one limb of y
    parts = _contiguous(RN, [130, 270, 200]) if P == 3 else _contiguous(RN, [333, 267])
    got = parallel.emulate_train_regressor(_shards(X, y, parts), RN, num_trees=RT, max_depth=DEPTH, seed=4,
                                           tree_chunk=chunk)
    assert got.inner_threshold.dtype == np.float64 and _bytes(got) == _bytes(_single(("reg", f64)))


def test_sampled_thresholds_across_block_boundaries(cuda):
    from dal import parallel
    from dal import random_forest as rf

    assert rf.split_sample_rows(BN, 32, 5) is not None  # the sample is drawn, not every row
    parts = _contiguous(BN, [1100, 5000, 5900])
    X, y = _class_pool(2, BN, BD, seed=23)
    got = parallel.emulate_train_classifier(_shards(X, y, parts), BN, num_trees=BT, max_depth=BDEPTH, seed=5)
    assert _bytes(got) == _bytes(_single(("big_class", None)))
    X, y = _reg_pool(False, BN, BD, seed=24)
    got = parallel.emulate_train_regressor(_shards(X, y, parts), BN, num_trees=BT, max_depth=BDEPTH, seed=6)
    assert _bytes(got) == _bytes(_single(("big_reg", None)))


def test_sharded_models_predict_as_the_single_device_models(cuda):
    from dal import parallel
    from dal import random_forest as rf

    probe = _class_pool(2, 256, D, seed=25)[0]
    for C in (2, 3):
        a, b = rf.predict(_fit_class(C, _interleaved(N, 3)), probe), rf.predict(_single(("class", C)), probe)
        assert all(u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() for u, v in zip(a, b))
    X, y = _reg_pool(False)
    got = parallel.emulate_train_regressor(_shards(X, y, _contiguous(RN, [130, 270, 200])), RN, num_trees=RT,
                                           max_depth=DEPTH, seed=4)
    probe = _reg_pool(False, 256, RD, seed=26)[0]
    assert rf.predict_regression(got, probe).cpu().numpy().tobytes() == \
        rf.predict_regression(_single(("reg", False)), probe).cpu().numpy().tobytes()


def test_bad_positions_raise(cuda):
    X, y = _class_pool(2)
    parts = _contiguous(N, [300, 300])
    parts[1] = parts[1].copy()
    parts[1][0] = 0  # position 0 twice, position 300 missing
    with pytest.raises(ValueError, match="exactly once"):
        _fit_class(2, parts)


# ---------------------------------------------------- a one-rank RCCL group --
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(port, q):
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, os.path.join(repo, "distributed-active-learning_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from dal import parallel
        from dal import random_forest as rf

        comm = parallel.TorchComm()
        out = {"backend": comm.backend}
        pos = np.arange(N)
        for C in (2, 3):
            X, y = _class_pool(C)
            kw = dict(num_trees=T, max_depth=DEPTH, seed=3, num_classes=C)
            out["class", C] = (_bytes(parallel.train_classifier(X, y, pos, N, comm, **kw)),
                               _bytes(rf.train_classifier(X, y, **kw)))
        X, y = _reg_pool(False)
        kw = dict(num_trees=RT, max_depth=DEPTH, seed=4)
        out["reg"] = (_bytes(parallel.train_regressor(X, y, np.arange(RN), RN, comm, **kw)),
                      _bytes(rf.train_regressor(X, y, **kw)))
        torch.cuda.synchronize()
        q.put(out)
    except Exception:  # surface worker failures instead of a queue timeout
        import traceback

        q.put(traceback.format_exc())
        raise
    finally:
        dist.destroy_process_group()


def test_rccl_world1_fits_equal_the_single_device_fits(cuda):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    assert p.exitcode == 0
    assert out["backend"] == "nccl"
    for key in (("class", 2), ("class", 3), "reg"):
        assert out[key][0] == out[key][1], key
