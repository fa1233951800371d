"""Incremental density exclusion on the GPU: PoolState.exclude (the density
downdate kernel, the repaired flags / operands / column-sum partials), the
dw.LABELED sentinel, run_loop(density_over="unlabeled") and the sharded
exclude, against a fresh PoolState of E u Delta and the oracle.

Pools: the smallest at which each slice width, the row padding and the Delta
tiling can go wrong -- 1,500 x 30 (d_pad 32, n not a multiple of 256), 512 x 64
(KS 64), 4,096 x 256 (KS 128, a 256-feature register chunk; also with the int8
and the fp4 form of the Gram).  E = range(10) with the density cached."""
import functools

import numpy as np
import pytest

import multiclass_dw_reference as DW
from conftest import golden_forest, load_golden
from dal import _lib
from dal.forest import Forest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

E0 = np.arange(10)
K = 25

POOLS = [
    ("synthetic_1500x30_T100.npz", {}),
    ("synthetic_512x64_T10.npz", {}),
    ("synthetic_4096x256_T10.npz", {}),
    ("synthetic_4096x256_T10.npz", {"gram_i8": True}),
    ("synthetic_4096x256_T10.npz", {"gram_fp4": True}),
]
POOL_IDS = ["1500x30", "512x64", "4096x256", "4096x256-i8", "4096x256-fp4"]


def _deltas(n):
    """The batches of one case: a list of successive exclude() arguments."""
    last0 = (n - 1) // 256 * 256  # first row of the last (partial) 256-row chunk
    step = max((n - 20) // 257, 1)
    tail = [n - 1, last0, last0 + 7, (last0 + n) // 2]
    return {
        "one": [[n // 2]],
        "ten": [list(range(300, 310))],
        "spread257": [list(12 + step * np.arange(257))],  # several chunks, five LDS tiles of Delta
        "tail": [tail],
        "dups_and_E": [[3, 3, 9, n // 3, n // 3, n // 3 + 1]],
        "two_calls": [list(range(300, 310)), tail + [305]],
    }


CASES = ["one", "ten", "spread257", "tail", "dups_and_E", "two_calls"]


class Ref:
    """A golden pool with its forests and per-E oracle quantities (computed once)."""

    def __init__(self, name):
        g = load_golden(name)
        self.X = g["X"]
        self.n, self.d = self.X.shape
        self.of = golden_forest(g)
        self.F = Forest.from_nodes(self.of.feature, self.of.threshold, self.of.left, self.of.right, self.of.value,
                                   self.of.roots)
        self.F3 = Forest.synthetic(10, 4, self.d, seed=5, n_classes=3)

    @functools.lru_cache(maxsize=None)
    def at(self, union_bytes):
        union = np.frombuffer(union_bytes, dtype=np.int64)
        dens = O.density_canonical(self.X, union)
        unl = np.setdiff1d(np.arange(self.n), union)
        _, idx, sc = O.density_select(self.X, unl, self.of, K, 1.0, union, density=dens)
        _, idx3, sc3, _ = DW.select(self.X, unl, self.F3, K, density=dens)
        for a in (dens, idx, sc, idx3, sc3):
            a.setflags(write=False)
        return dens, unl, (idx, sc), (idx3, sc3)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return Ref(name)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(_np(a) if hasattr(a, "cpu") else a, dtype=np.float64).view(np.uint64)


def _warm_state(cuda, ref, form, excluded=E0):
    from dal.engine import PoolState

    st = PoolState(ref.X, excluded=excluded, device=cuda, **form)
    st.density_fixed()
    st.colsum()
    return st


def _run_case(cuda, ref, form, batches):
    """exclude() the batches on a warm state: (state, union, expected bound)."""
    from dal.engine import density_error

    lib = _lib.load()
    st = _warm_state(cuda, ref, form)
    addr = st._density.data_ptr()
    err = 0.0
    bound = density_error(st)
    union = E0
    for b in batches:
        new = np.setdiff1d(np.unique(b), union)
        assert new.size <= _lib.DAL_DOWNDATE_MAX_ROWS
        err += float(lib.dal_density_downdate_error_bound(int(new.size), st.d_pad))
        assert st.exclude(b) == new.size
        union = np.union1d(union, new)
    assert st._density.data_ptr() == addr  # lowered in place
    assert st.exclude(batches[-1]) == 0    # nothing new: nothing changes
    return st, union, bound + err


def _same_selection(sel, ref_pair):
    assert np.array_equal(_np(sel.indices), ref_pair[0])
    assert np.array_equal(_bits(sel.selected_scores), _bits(ref_pair[1]))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_exclude_equals_fresh_pool(cuda, pool, case):
    import torch

    from dal import density_weighting as dw
    from dal.engine import density_error

    name, form = pool
    ref = _ref(name)
    batches = _deltas(ref.n)[case]
    st, union, bound = _run_case(cuda, ref, form, batches)
    dens, unl, sel_ref, sel3_ref = ref.at(union.tobytes())
    fresh = _warm_state(cuda, ref, form, excluded=union)
    assert (st.gram_i8, st.gram_fp4) == (fresh.gram_i8, fresh.gram_fp4) == \
        (bool(form.get("gram_i8")), bool(form.get("gram_fp4")))

    # 1. E and the flags
    assert np.array_equal(st.excluded, union) and np.array_equal(fresh.excluded, union)
    assert torch.equal(st.flags, fresh.flags)
    # 2. byte-identical caches
    assert np.array_equal(_bits(st.colsum()), _bits(fresh.colsum()))
    assert torch.equal(st.colsum_partials(), fresh.colsum_partials())
    sep = _np(st.density("separable"))
    assert np.array_equal(_bits(sep), _bits(fresh.density("separable")))
    assert np.array_equal(_bits(sep), _bits(dens))
    assert torch.equal(st.gram_operand(), fresh.gram_operand())
    if st.gram_i8:
        assert st._split_i8 is not None and torch.equal(st._split_i8, fresh.gram_operand_i8())
    if st.gram_fp4:
        assert st._split_fp4 is not None and torch.equal(st._split_fp4, fresh.gram_operand_fp4())
    # 3. the lowered Gram density within the summed bounds
    assert density_error(st) == bound
    keep = ~np.isnan(dens)
    got = _np(st.density("gram"))
    assert np.array_equal(np.isnan(got), ~keep)
    err = np.abs(got[keep] - dens[keep]).max()
    print(f"{name} {form} {case}: max |gram - canonical| = {err:.3e}, bound {bound:.3e}, "
          f"fresh pool's bound {density_error(fresh):.3e}")
    assert err <= bound
    # 4. run-to-run identical
    again, _, _ = _run_case(cuda, ref, form, batches)
    assert torch.equal(again.density_fixed(), st.density_fixed())
    # 5. selections: the oracle's and the fresh pool's, twice (the rebuilt warm plan is replayed)
    for _ in range(2):
        _same_selection(dw.select(st, unl, ref.F, K), sel_ref)
        _same_selection(dw.select_multiclass(st, unl, ref.F3, K), sel3_ref)
    _same_selection(dw.select(fresh, unl, ref.F, K), sel_ref)
    _same_selection(dw.select_multiclass(fresh, unl, ref.F3, K), sel3_ref)
    # the LABELED sentinel from the pre-exclude state takes the same path
    pre = _warm_state(cuda, ref, form)
    addr = pre._density.data_ptr()
    for _ in range(2):
        _same_selection(dw.select(pre, unl, ref.F, K, excluded_idx=dw.LABELED), sel_ref)
    assert pre._density.data_ptr() == addr and np.array_equal(pre.excluded, union)
    assert torch.equal(pre.density_fixed(), st.density_fixed()) or len(batches) > 1  # (one batch: the same downdate)
    _same_selection(dw.select_multiclass(ref.X, unl, ref.F3, K, excluded_idx=dw.LABELED, device=cuda), sel3_ref)


@pytest.mark.parametrize("pool", POOLS[:3], ids=POOL_IDS[:3])
def test_downdate_bytes_do_not_depend_on_the_grid(cuda, pool):
    """The kernel called directly with three grids: identical acc bytes, and
    the decrement equals the fp64 cosine sums within the downdate's bound."""
    from dal.engine import _ptr, _stream

    name, form = pool
    ref = _ref(name)
    lib = _lib.load()
    st = _warm_state(cuda, ref, form)
    chunk = np.setdiff1d(np.unique(_deltas(ref.n)["spread257"][0] + [ref.n - 1]), E0)
    delta = st.delta_operand(chunk)
    assert delta.shape[0] % _lib.DAL_DOWNDATE_TILE == 0 and delta.shape[0] >= chunk.size
    outs = []
    for grid in (0, 1, 3):
        acc = st.density_fixed().clone()
        _lib.call("dal_density_downdate", _ptr(st.gram_operand()), st.n_pad, st.d_pad, _ptr(delta), int(chunk.size),
                  _ptr(acc), grid, _stream(cuda))
        outs.append(_np(acc))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    dec = (_np(st.density_fixed()) - outs[0])[: ref.n].astype(np.float64) / _lib.DAL_FIXED_SCALE
    U = O.l2_normalize(ref.X)
    want = U @ U[chunk].sum(axis=0)
    keep = ~np.isin(np.arange(ref.n), E0)  # (E's operand rows are zero: their decrement is 0)
    bound = lib.dal_density_downdate_error_bound(int(chunk.size), st.d_pad)
    err = np.abs(dec[keep] - want[keep]).max()
    print(f"{name}: max |decrement - cosine sums| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.all(dec[~keep] == 0.0)
    assert np.array_equal(outs[0][ref.n:], _np(st.density_fixed())[ref.n:])  # padding rows: zero operand


def test_exclude_longer_than_one_downdate(cuda):
    """More rows than DAL_DOWNDATE_MAX_ROWS: chunked, one bound per chunk."""
    import torch

    from dal.engine import density_error

    ref = _ref("synthetic_4096x256_T10.npz")
    lib = _lib.load()
    st = _warm_state(cuda, ref, {})
    cold = density_error(st)
    rows = np.arange(100, 100 + _lib.DAL_DOWNDATE_MAX_ROWS + 37)
    assert st.exclude(rows) == rows.size
    want = 0.0
    for m in (_lib.DAL_DOWNDATE_MAX_ROWS, 37):
        want += float(lib.dal_density_downdate_error_bound(m, st.d_pad))
    assert density_error(st) == cold + want
    union = np.union1d(E0, rows)
    fresh = _warm_state(cuda, ref, {}, excluded=union)
    assert torch.equal(st.gram_operand(), fresh.gram_operand())
    assert np.array_equal(_bits(st.colsum()), _bits(fresh.colsum()))
    dens = O.density_canonical(ref.X, union)
    keep = ~np.isnan(dens)
    assert np.abs(_np(st.density("gram"))[keep] - dens[keep]).max() <= density_error(st)
    # the same E again keeps the lowered density and therefore its bound ...
    st.set_excluded(union)
    assert st._density is not None and density_error(st) == cold + want
    # ... clear_caches and a different E return to the cold rule
    st.clear_caches()
    assert density_error(st) == density_error(fresh)
    st.exclude(rows[:5] + 2000)
    assert st._density is None  # (no cached density: delegated)
    st.density_fixed()
    st.exclude([3000])
    assert density_error(st) > density_error(_warm_state(cuda, ref, {}, excluded=st.excluded))
    st.set_excluded(E0)
    assert density_error(st) == cold


def test_exclude_delegates_and_validates(cuda):
    """No cached density, or gram "f32": set_excluded(E u Delta); an index out
    of range raises set_excluded's ValueError and changes nothing."""
    from dal.engine import PoolState, density_error

    ref = _ref("synthetic_512x64_T10.npz")
    st = PoolState(ref.X, excluded=E0, device=cuda)
    assert st.exclude([20, 21, 3]) == 2 and st._density is None and st._density_cols is None
    assert np.array_equal(st.excluded, np.union1d(E0, [20, 21]))
    st.density_fixed()
    for bad in ([ref.n], [-1], [5, ref.n + 7]):
        with pytest.raises(ValueError, match="excluded indices must lie in"):
            st.exclude(bad)
    assert st.excluded.size == 12 and st._downdate_err == 0.0
    f32 = PoolState(ref.X, excluded=E0, device=cuda, gram="f32")
    f32.density_fixed()
    assert f32.exclude([40]) == 1 and f32._density is None
    fresh = PoolState(ref.X, excluded=np.union1d(E0, [40]), device=cuda, gram="f32")
    assert density_error(f32) == density_error(fresh)
    assert np.array_equal(_np(f32.density_fixed()), _np(fresh.density_fixed()))


@pytest.mark.parametrize("strategy", ["density", "information_density"])
def test_loop_over_the_unlabeled_pool(cuda, strategy):
    """run_loop(density_over="unlabeled"): every step's E is the current
    labeled set -- the same loop with the oracle as select_fn."""
    from dal import loop

    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"], g["y"]
    n = X.shape[0]
    seen = []

    def oracle_select(strategy, pool, unlabeled, rf, k):
        labeled = np.setdiff1d(np.arange(n), unlabeled)
        seen.append(labeled.size)
        if strategy == "density":
            return O.density_select(pool, unlabeled, O.forest_from_sklearn(rf), k, 1.0, labeled)[1]
        F = Forest.from_sklearn(rf, multiclass=True)
        return DW.select(pool, unlabeled, F, k, density=O.density_canonical(pool, labeled))[1]

    kw = dict(strategy=strategy, window_size=10, max_iterations=5, trainer="sklearn", density_over="unlabeled")
    ref = loop.run_loop(X, y, X, y, select_fn=oracle_select, **kw)
    got = loop.run_loop(X, y, X, y, device=cuda, **kw)
    assert seen == [10, 20, 30, 40, 50]
    assert got.log == ref.log
    assert len(got.labeled_history) == 5
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_sharded_exclude(cuda, world):
    """emulate_exclude over 1..4 shards of the 1,500 x 30 pool (4: the last
    shard is empty; 3: the last holds 476 rows): the next selection equals the
    single-device one and the oracle, the density slices are the single
    device's bytes and every selector's global column sum a fresh pool's."""
    import torch

    from dal import density_weighting as dw
    from dal import parallel

    ref = _ref("synthetic_1500x30_T100.npz")
    n = ref.n
    delta = [12, 511, 512, 700, 1023, 1024, 1290, n - 1, n - 1, 3]
    union = np.union1d(E0, delta)
    dens, unl, sel_ref, _ = ref.at(union.tobytes())
    sels = []
    for r in range(world):
        lo, hi, _ = parallel.shard_range(n, world, r)
        sels.append(parallel.ShardedSelector(ref.X[lo:hi], n, r, world, excluded=E0, device=cuda))
    parallel.emulate(sels, np.arange(10, n), ref.F, K, mode="dw")  # the cold step: densities cached
    addrs = [s._density.data_ptr() for s in sels]
    assert parallel.emulate_exclude(sels, delta) == union.size - E0.size
    assert [s._density.data_ptr() for s in sels] == addrs
    assert parallel.emulate_exclude(sels, delta) == 0
    one = _warm_state(cuda, ref, {})
    one.exclude(delta)
    fresh = _warm_state(cuda, ref, {}, excluded=union)
    for s in sels:
        assert np.array_equal(s.state.excluded, union)
        assert np.array_equal(_bits(s.global_colsum(s._parts_full)), _bits(fresh.colsum()))
        assert s._plans == {}
    total = torch.cat([s._density[: s.state.n] for s in sels])
    assert torch.equal(total, one.density_fixed()[:n])
    assert torch.equal(torch.cat([s.state.flags for s in sels]), fresh.flags)
    for _ in range(2):
        idx, sc = parallel.emulate(sels, unl, ref.F, K, mode="dw")
        assert np.array_equal(_np(idx), sel_ref[0]) and np.array_equal(_bits(sc), _bits(sel_ref[1]))
    _same_selection(dw.select(one, unl, ref.F, K), sel_ref)


SHARDED_DELTA = [12, 511, 512, 700, 1023, 1024, 1290, 1499, 1499, 3]  # test_sharded_exclude's, n = 1,500
BIG_N, BIG_D, BIG_K = 5000, 64, 40                                     # test_gpu_multiprocess.py's pool
BIG_DELTA = np.arange(50, BIG_N, 4)                                    # 1,238 new rows: two downdate chunks


def _pair(idx, sc):
    return _np(idx), _np(sc)


def _exclude_rank(rank, world):
    """parallel.exclude on one of two ranks sharing cuda:0 (collectives over
    gloo, counted).  Rank 0 also runs the big delta through emulate_exclude
    over the same two shards and through the single-device PoolState.exclude."""
    import torch

    from dal import density_weighting as dw
    from dal import parallel
    from sharded_comm import CountingComm

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    comm = CountingComm()
    out = {}

    def shard(X, n, r, **kw):
        lo, hi, _ = parallel.shard_range(n, world, r)
        return parallel.ShardedSelector(X[lo:hi], n, r, world, excluded=E0, device=dev, **kw)

    # -- the 1,500 x 30 pool: a delta over both shards with a repeat and a member of E
    ref = _ref("synthetic_1500x30_T100.npz")
    n = ref.n
    sel = shard(ref.X, n, rank)
    parallel.select(sel, comm, np.arange(10, n), ref.F, K, mode="dw")  # the cold step: density cached
    addr = sel._density.data_ptr()
    comm.take()
    out["new"] = parallel.exclude(sel, comm, SHARDED_DELTA)
    out["warm_counts"] = comm.take()
    out["plans"] = dict(sel._plans)
    out["again"] = parallel.exclude(sel, comm, SHARDED_DELTA)
    out["again_counts"] = comm.take()
    out["in_place"] = sel._density.data_ptr() == addr
    unl = np.setdiff1d(np.arange(n), np.union1d(E0, SHARDED_DELTA))
    out["next"] = [_pair(*parallel.select(sel, comm, unl, ref.F, K, mode="dw")) for _ in range(2)]
    comm.take()
    out["cold_new"] = parallel.exclude(shard(ref.X, n, rank), comm, [20, 21, 3])  # no cached density
    out["cold_counts"] = comm.take()
    # -- more new rows than one downdate takes: the chunk loop runs twice
    X = O.synthetic_pool(BIG_N, BIG_D, seed=21)
    F = Forest.synthetic(10, 4, BIG_D, seed=1)
    unl = np.setdiff1d(np.arange(BIG_N), np.union1d(E0, BIG_DELTA))
    sel = shard(X, BIG_N, rank)
    parallel.select(sel, comm, np.arange(10, BIG_N), F, BIG_K, mode="dw")
    comm.take()
    out["big_new"] = parallel.exclude(sel, comm, BIG_DELTA)
    out["big_counts"] = comm.take()
    out["big"] = _pair(*parallel.select(sel, comm, unl, F, BIG_K, mode="dw"))
    if rank == 0:
        sels = [shard(X, BIG_N, r) for r in range(world)]
        parallel.emulate(sels, np.arange(10, BIG_N), F, BIG_K, mode="dw")
        out["big_emulated_new"] = parallel.emulate_exclude(sels, BIG_DELTA)
        out["big_emulated"] = _pair(*parallel.emulate(sels, unl, F, BIG_K, mode="dw"))
        from dal.engine import PoolState

        one = PoolState(X, excluded=E0, device=dev)
        one.density_fixed()
        one.colsum()
        out["big_one_new"] = one.exclude(BIG_DELTA)
        s = dw.select(one, unl, F, BIG_K)
        out["big_one"] = _pair(s.indices, s.selected_scores)
    return out


def test_exclude_on_two_ranks(cuda):
    """parallel.exclude over a real group: counts, the density lowered in
    place, the plans dropped, the next selections the reference's bytes; a
    delta of two chunks equals emulate_exclude's and the single device's step;
    one all-gather per chunk and one of the partials when warm, none cold."""
    from sharded_comm import run_ranks

    ref = _ref("synthetic_1500x30_T100.npz")
    assert ref.n == 1500
    union = np.union1d(E0, SHARDED_DELTA)
    _, _, sel_ref, _ = ref.at(union.tobytes())
    assert BIG_DELTA.size > _lib.DAL_DOWNDATE_MAX_ROWS and BIG_DELTA.size <= 2 * _lib.DAL_DOWNDATE_MAX_ROWS
    res = run_ranks(_exclude_rank, 2)
    for out in res:
        assert out["new"] == union.size - E0.size and out["again"] == 0
        assert out["warm_counts"] == (2, 0) and out["again_counts"] == (0, 0)  # one chunk + the partials
        assert out["in_place"] and out["plans"] == {}
        for idx, sc in out["next"]:
            assert np.array_equal(idx, sel_ref[0]) and np.array_equal(_bits(sc), _bits(sel_ref[1]))
        assert out["cold_new"] == 2 and out["cold_counts"] == (0, 0)
        assert out["big_new"] == BIG_DELTA.size and out["big_counts"] == (3, 0)  # two chunks + the partials
        for name in ("big_emulated", "big_one"):
            assert res[0][name + "_new"] == BIG_DELTA.size
            assert np.array_equal(out["big"][0], res[0][name][0]), name
            assert np.array_equal(_bits(out["big"][1]), _bits(res[0][name][1])), name
