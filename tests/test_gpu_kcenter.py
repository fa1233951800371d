"""Greedy k-center (farthest-first) batch selection on the GPU
(dal.similarity.kcenter_select, dal.parallel.emulate_kcenter /
kcenter_select_sharded): indices and fp64 pick-time values bit-exact against
the numpy restatement of the canonical definition (tests/kcenter_reference.py),
the fp32 state within dal_kcenter_error_bound(d), equality with k successive
single-pick diversity selections, ties, contender floods, edge cases and
shards."""
import os
import socket

import numpy as np
import pytest

import kcenter_reference as KR
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(2000, 64, 20, 8, 60), (1500, 128, 16, 4, 16), (1200, 256, 12, 5, 40)]  # n, d, clusters, m, k

_REF = {}


def _np(t):
    return t.detach().cpu().numpy()


def _case(shape):
    """The clustered pool of a shape and its reference selection, computed once."""
    if shape not in _REF:
        n, d, clusters, m, k = shape
        X = KR.clustered_pool(n, d, clusters, seed=n + d)
        _REF[shape] = (X, KR.kcenter_reference(X, np.arange(m), k, np.arange(m, n)))
    return _REF[shape]


def _assert_selection(sel, ref):
    assert np.array_equal(_np(sel.indices), ref[0])
    assert _np(sel.selected_scores).tobytes() == ref[1].tobytes()


@pytest.mark.parametrize("shape", SHAPES)
def test_kcenter_bit_exact_and_state_within_bound(cuda, shape):
    from dal import _lib
    from dal import similarity as sim

    n, d, clusters, m, k = shape
    X, ref = _case(shape)
    # the test separates the two rules: the one-shot batch shares few rows with the greedy one
    top_idx, _ = O.diversity_select_canonical(X, np.arange(m), k, candidates=np.arange(m, n))
    assert np.intersect1d(top_idx, ref[0]).size <= k // 4
    assert np.unique(ref[0] % clusters).size > np.unique(top_idx % clusters).size
    sel = sim.kcenter_select(X, np.arange(m), k, candidates=np.arange(m, n), device=cuda)
    _assert_selection(sel, ref)
    assert np.all(np.diff(_np(sel.selected_scores)) >= 0)
    # the fp32 state of EVERY row after the last pick (the steps object keeps it)
    st = sim.HipKCenterSteps(cuda)
    st.prepare(X, 0, X[:m], np.arange(m, n))
    st.begin(k, select=True)
    idx, sc, scores = st.finish()
    assert np.array_equal(_np(idx), ref[0]) and _np(sc).tobytes() == ref[1].tobytes()
    bound = _lib.load().dal_kcenter_error_bound(d)
    err = np.abs(_np(st.m32).astype(np.float64) - ref[2]).max()
    print(f"n={n} d={d}: max |m32 - m| = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound
    assert np.array_equal(_np(scores), _np(st.m32)[m:]) and np.array_equal(_np(sel.scores), _np(scores))


def test_kcenter_equals_successive_single_picks(cuda):
    from dal import similarity as sim

    n, d, clusters, m, _ = SHAPES[1]
    k = 12
    X, _ = _case(SHAPES[1])
    sel = sim.kcenter_select(X, np.arange(m), k, candidates=np.arange(m, n), device=cuda)
    lab, cand, idx, sc = list(range(m)), list(range(m, n)), [], []
    for _ in range(k):
        one = sim.diversity_select(X, np.asarray(lab), 1, candidates=np.asarray(cand), device=cuda)
        p = int(one.indices[0])
        idx.append(p)
        sc.append(float(one.selected_scores[0]))
        lab.append(p)
        cand.remove(p)
    assert _np(sel.indices).tolist() == idx
    assert _np(sel.selected_scores).tobytes() == np.asarray(sc).tobytes()


def test_kcenter_ties_take_the_lower_index(cuda):
    from dal import similarity as sim

    n, d, m, k = 1500, 64, 8, 30
    X = O.bf16_round(O.synthetic_pool(n, d, seed=3))
    far = np.zeros(d, dtype=np.float32)
    far[0] = 1.0  # a corner of the positive orthant: the smallest max-cosine of the pool
    copies = np.concatenate([np.arange(100, 110), np.arange(1200, 1210)])  # two ranges, two blocks
    X[copies] = far
    ref = KR.kcenter_reference(X, np.arange(m), k, np.arange(m, n))
    sel = sim.kcenter_select(X, np.arange(m), k, candidates=np.arange(m, n), device=cuda)
    _assert_selection(sel, ref)
    picks = _np(sel.indices)
    assert picks[0] == 100
    assert np.intersect1d(picks[1:], copies).size == 0  # the other copies now hold the largest value


@pytest.mark.parametrize("case", ["identical", "near_ties"])
def test_kcenter_many_contenders(cuda, case):
    """5,000 identical least-similar rows (every one a contender of the first
    step) and 5,000 distinct near-tied rows (contenders at every step)."""
    from dal import similarity as sim

    n, d, m, k = 12000, 64, 256, 30
    X = O.bf16_round(O.synthetic_pool(n, d, seed=11))
    if case == "identical":
        far = np.zeros(d, dtype=np.float32)
        far[0] = 1.0
        X[3000:8000] = far
    else:
        rng = np.random.default_rng(5)
        near = np.zeros((5000, d), dtype=np.float32)
        near[:, 0] = 1.0
        rows = np.arange(5000)
        near[rows, rng.integers(1, d, 5000)] += rng.integers(1, 9, 5000) * 2.0 ** -10
        near[rows, rng.integers(1, d, 5000)] += rng.integers(1, 9, 5000) * 2.0 ** -12
        X[3000:8000] = O.bf16_round(near)
    ref = KR.kcenter_reference(X, np.arange(m), k, np.arange(m, n))
    sel = sim.kcenter_select(X, np.arange(m), k, candidates=np.arange(m, n), device=cuda)
    _assert_selection(sel, ref)
    if case == "identical":
        assert ref[0][0] == 3000


def test_kcenter_edge_cases(cuda):
    from dal import similarity as sim

    n, d, clusters, m, _ = SHAPES[0]
    X, _ = _case(SHAPES[0])
    # a candidate subset plus foreign indices
    cand = np.concatenate([np.arange(m, n, 3), np.arange(n, n + 50)])
    ref = KR.kcenter_reference(X, np.arange(m), 25, cand)
    sel = sim.kcenter_select(X, np.arange(m), 25, candidates=cand, device=cuda)
    _assert_selection(sel, ref)
    assert sel.scores.shape[0] == np.arange(m, n, 3).size
    # two runs: identical bytes
    again = sim.kcenter_select(X, np.arange(m), 25, candidates=cand, device=cuda)
    for a in ("indices", "selected_scores", "scores"):
        assert _np(getattr(sel, a)).tobytes() == _np(getattr(again, a)).tobytes()
    # k > |C|: |C| picks
    few = np.array([40, 41, 900, 1999, n + 7])
    ref = KR.kcenter_reference(X, np.arange(m), 10, few)
    sel = sim.kcenter_select(X, np.arange(m), 10, candidates=few, device=cuda)
    assert sel.indices.shape[0] == 4
    _assert_selection(sel, ref)
    # a zero-norm row
    Z = X.copy()
    Z[1234] = 0.0
    with pytest.raises(ValueError, match="zero-norm"):
        sim.kcenter_select(Z, np.arange(m), 5, device=cuda)


SIZES = {1: [2000], 2: [700, 1300], 3: [1100, 0, 900], 5: [300, 0, 1024, 75, 601]}


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_kcenter_shards_equal_the_single_device_bytes(cuda, P):
    import torch

    from dal import parallel
    from dal import similarity as sim

    n, d, clusters, m, k = SHAPES[0]
    X, ref = _case(SHAPES[0])
    single = sim.kcenter_select(X, np.arange(m), k, candidates=np.arange(m, n), device=cuda)
    bounds = np.concatenate([[0], np.cumsum(SIZES[P])])
    shards = [(torch.from_numpy(X[bounds[r]:bounds[r + 1]]).to(cuda), int(bounds[r])) for r in range(P)]
    sel = parallel.emulate_kcenter(shards, X[:m], k, candidates=np.arange(m, n),
                                   steps=lambda: sim.HipKCenterSteps(cuda))
    _assert_selection(sel, ref)
    for a in ("indices", "selected_scores", "scores"):
        assert _np(getattr(sel, a)).tobytes() == _np(getattr(single, a)).tobytes()


# ------------------------------------------------- a one-rank RCCL group --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


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

        n, d, clusters, m, k = SHAPES[1]
        X = KR.clustered_pool(n, d, clusters, seed=n + d)
        comm = parallel.TorchComm()
        sel = parallel.kcenter_select_sharded(torch.from_numpy(X).to(dev), 0, X[:m], k, comm,
                                              candidates=np.arange(m, n), device=dev)
        torch.cuda.synchronize()
        q.put({"backend": comm.backend, "indices": _np(sel.indices), "scores": _np(sel.selected_scores)})
    except Exception:  # surface worker failures instead of a queue timeout
        import traceback

        q.put(traceback.format_exc())
        raise
    finally:
        dist.destroy_process_group()


def test_kcenter_rccl_world1(cuda):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    assert p.exitcode == 0 and out["backend"] == "nccl"
    _, ref = _case(SHAPES[1])
    assert np.array_equal(out["indices"], ref[0]) and out["scores"].tobytes() == ref[1].tobytes()
