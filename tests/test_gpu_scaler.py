"""The exact StandardScaler on the GPU (csrc/scaler.hip, dal.dataset) against
the restatement in Python integers (tests/scaler_reference.py): mean, std and
every standardised value byte for byte, for any row order, chunking and
sharding; the refusals; the dataset classes and the LAL loop's start state.

Reference: lal_direct_mllib_implementation/classes/dataset.py:56-130, :163-173.
"""
import os
import socket

import numpy as np
import pytest

import scaler_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

# the smallest shapes at which the kernels can go wrong: one row (n - 1 == 0), row counts around a wave, column
# counts 1 (256 row lanes), 2, 3 and 30 (padded column tiles) and 257 (five tiles, the last with one column)
SHAPES = [(1, 1), (1, 30), (2, 2), (2, 257), (63, 3), (64, 30), (65, 1), (65, 257), (64, 3), (63, 257),
          (4097, 2), (4097, 30)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pool(n, d, seed):
    """U[0,1) in the even columns, 3 N(0,1) + 10 in the odd ones."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, d), dtype=np.float32)
    X[:, 1::2] = (3.0 * rng.standard_normal((n, d))[:, 1::2] + 10.0).astype(np.float32)
    return X


def _check_model(model, X, cuda, x_dev=None):
    mean, std = R.moments(X)
    assert model.n == X.shape[0]
    assert _same(model.mean, mean), (model.mean, mean)
    assert _same(model.std, std), (model.std, std)
    src = X if x_dev is None else x_dev
    for dtype in (np.float32, np.float64):
        z = model.transform(src, dtype=dtype, device=cuda)
        assert z.is_cuda and z.is_contiguous()
        assert _same(z.cpu().numpy(), R.transform(X, mean, std, dtype=dtype)), dtype


@pytest.mark.parametrize("n,d", SHAPES)
def test_fit_and_transform_bytes(cuda, n, d):
    from dal.dataset import StandardScaler

    X = _pool(n, d, seed=n * 1000 + d)
    _check_model(StandardScaler().fit(X, device=cuda), X, cuda)


def test_leading_dimension_and_block_straddle(cuda):
    import torch

    from dal import _lib
    from dal.dataset import StandardScaler

    # ld > d: a view of a wider device array, read and written with its own strides
    X = _pool(65, 30, seed=5)
    wide = torch.full((65, 37), float("nan"), dtype=torch.float32, device=cuda)
    wide[:, :30] = torch.from_numpy(X).to(cuda)
    view = wide[:, :30]
    assert view.stride(0) == 37
    _check_model(StandardScaler().fit(view), X, cuda, x_dev=view)
    # a row count that is no multiple of the rows of one block, over several blocks per column tile
    n, d = 1031, 3
    rpb = _lib.load().dal_scaler_rows_per_block(n, d)
    assert 0 < rpb < n and n % rpb
    X = _pool(n, d, seed=6)
    _check_model(StandardScaler().fit(X, device=cuda), X, cuda)


def _crafted(n=300):
    rng = np.random.default_rng(9)
    cols = [rng.random(n, dtype=np.float32),                                       # 0 ordinary
            np.full(n, 0.1, dtype=np.float32),                                     # 1 constant: std 0 -> +0.0
            (16777216.0 + (np.arange(n) % 3)).astype(np.float32),                  # 2 2^24 + {0, 1, 2} in fp32
            np.where(np.arange(n) % 4 == 0, -0.0, -rng.random(n) - 0.5).astype(np.float32),   # 3 negatives, -0.0
            np.zeros(n, dtype=np.float32),                                         # 4 all zero
            (rng.choice([2.0 ** -40, 2.0 ** 20], n) * rng.choice([-1.0, 1.5], n)).astype(np.float32),  # 5
            (3.0 * rng.standard_normal(n) + 10.0).astype(np.float32),              # 6 ordinary
            np.full(n, -0.0, dtype=np.float32)]                                    # 7 all -0.0
    return np.stack(cols, axis=1)


def test_crafted_columns(cuda):
    from dal.dataset import StandardScaler, scaler_limbs

    X = _crafted()
    low, top = R.column_format(X)
    k1, k2, q = scaler_limbs(low, top)
    # K is the pool's maximum (column 5), above what every other column needs
    assert (k1, k2) == (2, 4) and int(top[0]) - int(low[0]) <= 31 and int(top[2]) - int(low[2]) == 24
    model = StandardScaler().fit(X, device=cuda)
    _check_model(model, X, cuda)
    assert model.std[1] == 0.0 and model.std[4] == 0.0 and model.std[7] == 0.0
    assert model.mean[4] == 0.0 and not np.signbit(model.mean[4]) and not np.signbit(model.mean[7])
    z = model.transform(X, device=cuda).cpu().numpy()
    assert not np.isnan(z).any()
    for c in (1, 4, 7):
        assert not z[:, c].any() and not np.signbit(z[:, c]).any()                 # +0.0, never NaN or -0.0
    # without the mean / without the deviation
    for kw in ({"with_mean": False}, {"with_std": False}, {"with_mean": False, "with_std": False}):
        m = StandardScaler(**kw).fit(X, device=cuda)
        for dtype in (np.float32, np.float64):
            want = R.transform(X, model.mean, model.std, dtype=dtype, **kw)
            assert _same(m.transform(X, dtype=dtype, device=cuda).cpu().numpy(), want), (kw, dtype)


def test_refusals(cuda):
    import torch

    from dal import _lib
    from dal.dataset import StandardScaler, device_accumulate

    X = _pool(70, 3, seed=2)
    bad = X.copy()
    bad[:, 1] = 1.0
    bad[41, 1] = 1e-45                                                              # a subnormal beside 1.0
    with pytest.raises(_lib.DalError, match=r"status -3\): column 1 spans 150 bits"):
        StandardScaler().fit(bad, device=cuda)
    for v in (np.nan, np.inf, -np.inf):
        bad = X.copy()
        bad[69, 2] = v
        with pytest.raises(ValueError, match="finite"):
            StandardScaler().fit(bad, device=cuda)
    # a refused accumulate leaves the caller's cells as they were
    x = torch.from_numpy(X).to(cuda)
    cells = torch.arange(3 * 10, dtype=torch.int64, device=cuda).reshape(3, 10) - 7
    before = cells.clone()
    with pytest.raises(_lib.DalError, match="status -3"):
        device_accumulate(x, 70, 3, 3, np.zeros(3, np.int32), 1, 9, cells=cells)
    torch.cuda.synchronize()
    assert torch.equal(cells, before)
    # n == 0 is DAL_OK and leaves them untouched too
    q = torch.zeros(3, dtype=torch.int32, device=cuda)
    _lib.call("dal_scaler_accumulate", x.data_ptr(), 0, 3, 3, q.data_ptr(), 2, 8, cells.data_ptr(), None)
    torch.cuda.synchronize()
    assert torch.equal(cells, before)


def test_order_chunks_and_shards(cuda):
    import torch

    from dal import parallel
    from dal.dataset import StandardScaler

    X = np.concatenate([_crafted(1031), _pool(1031, 5, seed=8)], axis=1)
    mean, std = R.moments(X)
    n = X.shape[0]

    def same(m):
        return m.n == n and _same(m.mean, mean) and _same(m.std, std)

    s = StandardScaler()
    assert same(s.fit(X, device=cuda)) and same(s.fit(X, device=cuda))              # a repeated fit
    perm = np.random.default_rng(1).permutation(n)
    assert same(s.fit(X[perm], device=cuda))
    for parts in (1, 2, 3):
        assert same(s.fit(X, device=cuda, chunk_rows=-(-n // parts)))
    x = torch.from_numpy(X).to(cuda)
    for cuts in ([0, n], [0, 400, n], [0, 400, 400, n], [0, 0, 513, n]):            # 1, 2, 3 shards, empty ones too
        shards = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        assert same(parallel.emulate_fit_scaler(shards)), cuts


def test_checkerboard_and_from_text(cuda, tmp_path):
    from dal.dataset import Dataset, DatasetCheckerboard2x2, StandardScaler

    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"], g["y"]
    assert X.shape == (1000, 2) and X.dtype == np.float32
    model = StandardScaler().fit(X, device=cuda)
    _check_model(model, X, cuda)
    mean, std = R.moments(X)
    want = R.transform(X, mean, std)
    # through the text files of the reference's layout: features, then the 0/1 label
    Xt, yt = X[:300][::-1].copy(), y[:300][::-1].copy()
    for name, A, b in (("checkerboard2x2_train.txt", X, y), ("checkerboard2x2_test.txt", Xt, yt)):
        with open(tmp_path / name, "w") as f:
            for row, lab in zip(A, b):
                f.write(" ".join(repr(float(v)) for v in row) + f" {int(lab)}\n")
    train, test = str(tmp_path / "checkerboard2x2_train.txt"), str(tmp_path / "checkerboard2x2_test.txt")
    raw = Dataset.from_text(train, test, standardize=False)
    assert _same(raw.train_X, X) and np.array_equal(raw.train_y, y) and _same(raw.test_X, Xt)
    ds = Dataset.from_text(train, test, device=cuda)
    assert ds.train_X.is_cuda and _same(ds.train_X.cpu().numpy(), want)
    assert np.array_equal(ds.train_y, y) and np.array_equal(ds.test_y, yt)
    tm, tsd = R.moments(Xt)                                                        # "own": the test split's scaler
    assert _same(ds.test_scaler.mean, tm) and _same(ds.test_X.cpu().numpy(), R.transform(Xt, tm, tsd))
    ds2 = Dataset.from_text(train, test, test_scaler="train", device=cuda)
    assert ds2.test_scaler is ds2.train_scaler
    assert _same(ds2.test_X.cpu().numpy(), R.transform(Xt, mean, std))
    named = DatasetCheckerboard2x2(str(tmp_path), device=cuda)
    assert _same(named.train_X.cpu().numpy(), want) and _same(named.test_X.cpu().numpy(), ds.test_X.cpu().numpy())


def test_dataset_to_lal_loop(cuda):
    from dal import loop
    from dal.dataset import Dataset
    from dal.forest import RegressionForest

    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"], g["y"]
    ds = Dataset(X, y).standardize(device=cuda)
    known, unknown = ds.set_start_state(2, seed=3)
    assert y[known[0]] == 1 and y[known[1]] == 0 and unknown.size == 998
    mean, std = R.moments(X)
    host = R.transform(X, mean, std)
    model = RegressionForest.synthetic(7, 4, 5, seed=47)
    kw = dict(strategy="lal", lal_model=model, trainer="gpu", window_size=1, max_iterations=3, device=cuda,
              initial_labeled=known)
    got = loop.run_loop(ds.train_X, ds.train_y, **kw)
    ref = loop.run_loop(host, y, **kw)
    assert got.log == ref.log and got.log[0] == "labeled =  2  unlabeled =  998"
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(a, b) and not np.isin(a, known).any()


# ------------------------------------------------------------------- RCCL --
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

        comm = parallel.TorchComm()
        X = _crafted(517)
        m = parallel.fit_scaler(torch.from_numpy(X).to(dev), comm)
        torch.cuda.synchronize()
        q.put({"backend": comm.backend, "n": m.n, "mean": m.mean, "std": m.std})
    except Exception:  # surface worker failures instead of a queue timeout
        import traceback

        q.put(traceback.format_exc())
        raise
    finally:
        dist.destroy_process_group()


def test_rccl_world1_fit_scaler(cuda):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    assert p.exitcode == 0
    mean, std = R.moments(_crafted(517))
    assert out["backend"] == "nccl" and out["n"] == 517
    assert _same(out["mean"], mean) and _same(out["std"], std)
