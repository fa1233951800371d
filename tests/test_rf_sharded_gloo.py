"""Row-sharded forest training without a GPU: dal.parallel.train_classifier /
train_regressor and their emulate_* twins with the local HIP steps replaced
by the level-stepped restatement (tests/rf_sharded_reference.py), against the
one-piece references on the concatenated rows -- oracle.rf_oracle (binary),
rf_multiclass_reference (C classes), rf_regress_reference (regression) -- byte
for byte; and the argument checks of the level-step C ABI."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rf_multiclass_reference as RM
import rf_regress_reference as RR
import rf_sharded_reference as S
from dal import parallel
from dal import random_forest as rf
from oracle import rf_oracle

N, D, T, DEPTH, BINS, SEED = 90, 4, 3, 3, 8, 5
KINDS = ("binary", "multi", "regress")


def _pool(kind):
    rng = np.random.default_rng(11)
    X = np.round(rng.random((N, D)) * 9).astype(np.float32) / 4  # ten values per feature: bins tie
    if kind == "regress":
        y = X[:, 0].astype(np.float64) * 3 + rng.random(N) + 1e3
    else:
        C = 2 if kind == "binary" else 3
        y = ((X[:, 0] * 2 + X[:, 1] + rng.random(N) * 1.5).astype(np.int64) % C).astype(np.int64)
    return X, y


_REF = {}


def _reference(kind):
    """The one-piece fit of the whole pool, computed once: heap arrays in the models' layout."""
    if kind not in _REF:
        X, y = _pool(kind)
        if kind == "regress":
            w, sub = rf.bagging_inputs(N, D, T, DEPTH, SEED, rf.regression_subset_strategy(T))
            _REF[kind] = RR.train_regressor(X, y, w, sub, max_depth=DEPTH, max_bins=BINS)[2]
        elif kind == "binary":
            w, sub = rf.bagging_inputs(N, D, T, DEPTH, SEED)
            _, sf, st, lc = rf_oracle.train_classifier(X, y, w, sub, max_depth=DEPTH, max_bins=BINS)
            _REF[kind] = RM.heap_arrays(sf, st, lc)
        else:
            w, sub = rf.bagging_inputs(N, D, T, DEPTH, SEED)
            _, sf, st, lc = RM.train_classifier(X, y, w, sub, 3, max_depth=DEPTH, max_bins=BINS)
            _REF[kind] = RM.heap_arrays(sf, st, lc)
    return _REF[kind]


def _arrays(kind, model):
    if kind == "regress":
        return model.inner_feature, model.inner_threshold, model.leaf
    return model.inner, model.leaf


def _assert_equal(kind, model):
    for got, want in zip(_arrays(kind, model), _reference(kind)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _parts(scheme, P):
    if scheme == "contiguous":
        sizes = {1: [N], 2: [1, N - 1], 3: [7, 52, N - 59]}[P]
        return S.contiguous(N, sizes)
    if scheme == "interleaved":
        return S.interleaved(N, P)
    return S.interleaved(N, P, empty=P - 2)  # "empty": one rank holds no row


def _kwargs(kind):
    kw = dict(num_trees=T, max_depth=DEPTH, max_bins=BINS, seed=SEED)
    if kind == "multi":
        kw["num_classes"] = 3
    return kw


def _emulate(kind, shards, **extra):
    fn = parallel.emulate_train_regressor if kind == "regress" else parallel.emulate_train_classifier
    return fn(shards, N, steps=S.NumpySteps, **_kwargs(kind), **extra)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P,scheme", [(1, "contiguous"), (2, "contiguous"), (2, "interleaved"), (3, "contiguous"),
                                      (3, "interleaved"), (3, "empty")])
def test_emulate_equals_the_one_piece_reference(kind, P, scheme):
    X, y = _pool(kind)
    _assert_equal(kind, _emulate(kind, S.split_shards(X, y, _parts(scheme, P))))


def test_regressor_chunks_do_not_change_the_bytes():
    X, y = _pool("regress")
    shards = S.split_shards(X, y, _parts("interleaved", 2))
    for chunk in (1, 2):
        _assert_equal("regress", _emulate("regress", shards, tree_chunk=chunk))


@pytest.mark.parametrize("kind", KINDS)
def test_positions_with_a_duplicate_or_a_gap_raise(kind):
    X, y = _pool(kind)
    parts = _parts("contiguous", 3)
    dup = [parts[0], np.concatenate([parts[1][:-1], parts[0][:1]]), parts[2]]  # position 0 twice, one missing
    with pytest.raises(ValueError, match="exactly once"):
        _emulate(kind, S.split_shards(X, y, dup))
    gap = [parts[0], parts[1][:-1], parts[2]]
    with pytest.raises(ValueError, match="exactly once"):
        _emulate(kind, S.split_shards(X, y, gap))
    with pytest.raises(ValueError):
        _emulate(kind, [(X[:3], y[:3], np.array([0, 1, N]))] + S.split_shards(X, y, [np.arange(3, N)]))


def test_shards_of_different_width_or_dtype_raise():
    X, y = _pool("regress")
    parts = _parts("contiguous", 2)
    a, b = S.split_shards(X, y, parts)
    with pytest.raises(ValueError, match="feature count"):
        _emulate("regress", [a, (b[0][:, :3], b[1], b[2])])
    with pytest.raises(ValueError, match="dtype"):
        _emulate("regress", [a, (b[0].astype(np.float64), b[1], b[2])])


class _Recording(S.NumpySteps):
    seen = []

    def begin(self, job):
        _Recording.seen.append(job.fmt)
        super().begin(job)


def test_zero_label_shard_does_not_move_the_label_format():
    """A shard whose labels are all zero, and an empty one, next to labels
    1e6 + k 2^-10: the global (q, k) are those of the concatenated labels (an
    all-zero shard alone would report (0, 1))."""
    rng = np.random.default_rng(3)
    n = 40
    X = np.round(rng.random((n, 3)) * 5).astype(np.float32)
    y = np.concatenate([np.zeros(15), 1e6 + np.arange(25) * 2.0 ** -10])
    w, sub = rf.bagging_inputs(n, 3, 2, 2, 1, "all")
    parts = [np.arange(0, 15), np.zeros(0, dtype=np.int64), np.arange(15, n)]
    _Recording.seen = []
    got = parallel.emulate_train_regressor(S.split_shards(X, y, parts), n, max_depth=2, max_bins=8, weights=w,
                                           feature_subsets=sub, steps=_Recording)
    _, f_y, f_sq = rf.check_regression_labels(y, n)
    assert f_y == (-10, 1) and set(_Recording.seen) == {f_y + f_sq}
    assert rf.check_regression_labels(y[:15], 15)[1] == (0, 1)
    want = RR.train_regressor(X, y, w, sub, max_depth=2, max_bins=8)[2]
    for a, b in zip(_arrays("regress", got), want):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match="finite"):
        bad = y.copy()
        bad[20] = np.inf
        parallel.emulate_train_regressor(S.split_shards(X, bad, parts), n, max_depth=2, max_bins=8, weights=w,
                                         feature_subsets=sub, steps=S.NumpySteps)


# ------------------------------------------------------------ a gloo group --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _schemes(world):
    return ("contiguous", "interleaved") if world == 2 else ("contiguous", "empty")


def _run(rank, world, q):
    comm = parallel.TorchComm()
    out = {}
    for kind in KINDS:
        X, y = _pool(kind)
        fn = parallel.train_regressor if kind == "regress" else parallel.train_classifier
        for scheme in _schemes(world):
            p = _parts(scheme, world)[rank]
            m = fn(X[p], y[p], p, N, comm, steps=S.NumpySteps(), **_kwargs(kind))
            out[kind, scheme] = [a.tobytes() for a in _arrays(kind, m)]
    X, y = _pool("binary")
    p = _parts("contiguous", world)[rank]
    p = p[:-1] if rank == world - 1 else p  # a gap: every rank must raise
    try:
        parallel.train_classifier(X[p], y[p], p, N, comm, steps=S.NumpySteps(), **_kwargs("binary"))
        out["gap"] = "no error"
    except ValueError as e:
        out["gap"] = str(e)
    q.put((rank, out))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _run(rank, world, q)
    except Exception as e:  # surface worker failures instead of a queue timeout
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_group_equals_the_one_piece_reference(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out in res:
        assert not isinstance(out, str), out
        assert "exactly once" in out["gap"], (rank, out["gap"])
        for kind in KINDS:
            for scheme in _schemes(world):
                assert out[kind, scheme] == [a.tobytes() for a in _reference(kind)], (rank, kind, scheme)


# ------------------------------------------------------------------- C ABI --
def _device_buffers(n_bytes):
    """Real device buffers where a GPU is present (begin then resets a real
    workspace); without one every HIP call fails and a placeholder address is
    never touched."""
    if torch.cuda.is_available():
        t = torch.zeros(n_bytes + 256, dtype=torch.uint8, device="cuda")
        return t, ctypes.c_void_p((t.data_ptr() + 255) // 256 * 256)
    return None, ctypes.c_void_p(256)


TRAINERS = ("dal_rf_train", "dal_rf_train_multiclass", "dal_rf_train_regressor")


def _begin(lib, name, job, buf, depth=4, null=None, d=5, m=2, trees=10, ns=31, classes=3, ky=2, ksq=3, n=0):
    """*_begin over an empty shard (rows, labels and weights null)."""
    p = [job, buf, buf, buf, buf, buf, buf, buf]  # job thresholds n_splits subsets out0 out1 out2 ws
    if null is not None:
        p[null] = None
    job, thr, nsp, sub, o0, o1, o2, ws = p
    grow = (ns, None, sub, m, trees, depth, 1, 0.0)
    if name == "dal_rf_train_regressor":
        return lib.dal_rf_train_regressor_begin(job, None, n, d, None, thr, nsp, *grow, -60, ky, -110, ksq, o0, o1,
                                                o2, ws, 1 << 24, None)
    extra = (classes,) if name == "dal_rf_train_multiclass" else ()
    return getattr(lib, name + "_begin")(job, None, n, d, d, None, thr, nsp, *grow, *extra, o0, o1, ws, 1 << 24,
                                         None)


@pytest.mark.parametrize("name", TRAINERS)
def test_level_step_abi_rejects_before_any_hip_call(name):
    from dal import _lib

    lib = _lib.load()
    assert lib.dal_abi_version() == 10 and _lib.DAL_RF_JOB_BYTES == 512
    steps = [name + s for s in ("_begin", "_level_stats", "_level_split", "_finish", "_level_span")]
    for s in steps:
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    keep, buf = _device_buffers(1 << 24)
    job = ctypes.create_string_buffer(_lib.DAL_RF_JOB_BYTES)
    stats, split, finish, span = (getattr(lib, s) for s in steps[1:])
    ptr, kind, count = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int64()
    out = (ctypes.byref(ptr), ctypes.byref(kind), ctypes.byref(count))
    # a descriptor nothing filled
    assert stats(job, 0, None) == -1 and split(job, 0, None) == -1 and finish(job, None) == -1
    assert span(job, 0, *out) == -1 and stats(None, 0, None) == -1 and finish(None, None) == -1
    # begin: null pointers, a depth of 11, bad limbs, bad shapes -- all before a device call
    for i in (range(8) if name == "dal_rf_train_regressor" else (0, 1, 2, 3, 4, 5, 7)):  # the classifiers have two outputs
        assert _begin(lib, name, job, buf, null=i) == -1  # DAL_ERR_ARG
    assert _begin(lib, name, job, buf, depth=11) == -3 and _begin(lib, name, job, buf, depth=0) == -3
    assert _begin(lib, name, job, buf, n=-1) == -2 and _begin(lib, name, job, buf, m=6) == -2
    assert _begin(lib, name, job, buf, ns=255) == -2
    if name == "dal_rf_train_regressor":
        assert _begin(lib, name, job, buf, ky=9) == -3 and _begin(lib, name, job, buf, ksq=0) == -3
        assert _begin(lib, name, job, buf, d=200, m=104) == -3  # one node's cells above DAL_RF_SPLIT_LDS_BYTES
    if name == "dal_rf_train_multiclass":
        assert _begin(lib, name, job, buf, classes=33) == -3 and _begin(lib, name, job, buf, classes=1) == -3
    assert stats(job, 0, None) == -1  # a refused begin leaves no job behind
    # an empty shard is a legal job (DAL_OK on a device; without one the reset fails after the descriptor is written)
    assert _begin(lib, name, job, buf) == (0 if keep is not None else -4)
    for level in (-1, 5):  # outside [0, max_depth]
        assert stats(job, level, None) == -2 and split(job, level, None) == -2 and span(job, level, *out) == -2
    assert span(job, 2, None, *out[1:]) == -1
    other = TRAINERS[(TRAINERS.index(name) + 1) % 3]
    assert getattr(lib, other + "_level_stats")(job, 0, None) == -1  # another trainer's job
    # the span DESIGN.md states: T 2^l (C + m hb C) int32 / T 2^l (W + m hb W) int64, the totals alone at max_depth
    cell = {"dal_rf_train": 2, "dal_rf_train_multiclass": 3, "dal_rf_train_regressor": 1 + 2 + 3}[name]
    want_kind = _lib.DAL_RF_SPAN_I64 if name == "dal_rf_train_regressor" else _lib.DAL_RF_SPAN_I32
    for level in range(5):
        assert span(job, level, *out) == 0
        per_node = cell + (2 * 33 * cell if level < 4 else 0)
        assert kind.value == want_kind and count.value == 10 * (1 << level) * per_node
        size = 8 if want_kind == _lib.DAL_RF_SPAN_I64 else 4
        assert ptr.value % size == 0 and buf.value <= ptr.value and ptr.value + count.value * size <= buf.value + (1 << 24)
