"""Test-set evaluation on the GPU (csrc/forest_eval.hip, csrc/sq_error.hip,
dal.metrics): the joint table of dal_forest_evaluate cell for cell against the
restatement (tests/metrics_reference.py) in both kernel forms, rows on a
threshold, label and leaf bytes outside the classes, flags, accumulation, the
measures end to end on the checkerboard pools, the exact MSE, and
run_loop(measures=)."""
import math

import numpy as np
import pytest

import metrics_reference as R
from conftest import load_golden
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 65, 1000)  # one row, one short of a 64-row tile, one past it, many tiles and a ragged last one
BINARY = ("accuracy", "TN", "FP", "FN", "TP", "auc", "confusion")


def _pool(n, d, F, seed):
    """A synthetic pool with rows exactly on a root threshold (they go left)
    and one fp32 ulp above it (they go right)."""
    X = O.synthetic_pool(n, d, seed=seed).astype(np.float32)
    T = F.inner.shape[0]
    for i in range(min(n, 2 * T)):
        f = int(F.inner[i % T, 0, 0])
        thr = F.inner[i % T, 0, 1:2].view(np.float32)[0]
        X[i, f] = thr if i % 2 == 0 else np.nextafter(thr, np.float32(np.inf))
    return X


class _Case:
    """A pool on the device with row stride ldx > d, its blocked copy and the
    prepared forest; tables(...) runs dal_forest_evaluate in each form."""

    def __init__(self, cuda, X, F, pad=3):
        import torch

        from dal import _lib
        from dal._lib import call

        self.lib, self.cuda, self.F = _lib.load(), cuda, F
        self.n, self.d = X.shape
        self.ldx = self.d + pad
        self.x = torch.full((max(self.n, 1), self.ldx), float("nan"), dtype=torch.float32, device=cuda)
        self.x[:self.n, :self.d] = torch.from_numpy(X).to(cuda)
        self.S = torch.cuda.current_stream(cuda).cuda_stream
        self.C = int(F.n_classes)
        self.rule = int(self.lib.dal_forest_evaluate_blocked_rows(self.d, F.n_trees, F.depth, self.C))
        self.inner, self.leaf = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (F.inner, F.leaf))
        self.xb = self.prep = None
        if self.rule:
            self.xb = torch.empty(int(self.lib.dal_pool_blocked_floats(self.n, self.d)), dtype=torch.float32,
                                  device=cuda)
            call("dal_pool_blocked", self.x.data_ptr(), self.n, self.d, self.ldx, self.xb.data_ptr(), self.S)
            nb = int(self.lib.dal_forest_prep_bytes(self.d, F.n_trees, F.depth))
            assert nb > 0
            self.prep = torch.empty(nb, dtype=torch.uint8, device=cuda)
            call("dal_forest_prepare", self.inner.data_ptr(), self.leaf.data_ptr(), F.n_trees, F.depth, self.d,
                 self.prep.data_ptr(), nb, self.S)
        self.cells = int(self.lib.dal_forest_evaluate_cells(F.n_trees, self.C))

    def forms(self):
        return ("rows", "blocked") if self.rule else ("rows",)

    def run(self, form, labels, flags=None, hist=None, row0=0, n=None):
        """One call over rows [row0, row0 + n) into ``hist`` (a new zeroed
        table when None); row0 is a multiple of 64 for the blocked form."""
        import torch

        from dal._lib import call

        n = self.n - row0 if n is None else n
        if hist is None:
            hist = torch.zeros(self.cells, dtype=torch.int64, device=self.cuda)
        blocked = form == "blocked"
        assert not blocked or row0 % 64 == 0
        call("dal_forest_evaluate", self.x.data_ptr() + 4 * row0 * self.ldx,
             self.xb.data_ptr() + 4 * row0 * self.d if blocked else 0, self.prep.data_ptr() if blocked else 0,
             n, self.d, self.ldx, self.inner.data_ptr(), self.leaf.data_ptr(), self.F.n_trees, self.F.depth, self.C,
             labels.data_ptr() + row0, 0 if flags is None else flags.data_ptr() + row0, hist.data_ptr(), self.S)
        return hist

    def table(self, form, labels, flags=None):
        shape = (self.F.n_trees + 1, 2) if self.C == 2 else (self.C, self.C)
        return self.run(form, labels, flags).cpu().numpy().reshape(shape)


def _dev(cuda, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(cuda)


def _check_case(cuda, n, d, F, seed):
    X = _pool(n, d, F, seed)
    y = np.random.default_rng(seed + 1).integers(0, F.n_classes, n).astype(np.uint8)
    case = _Case(cuda, X, F)
    want = np.array(R.joint_table(F, X, y), dtype=np.int64)
    assert int(want.sum()) == n
    for form in case.forms():
        got = case.table(form, _dev(cuda, y))
        assert np.array_equal(got, want), (form, n, d, F.n_trees, F.n_classes)
    return case.rule


@pytest.mark.parametrize("d", [5, 30, 256])
@pytest.mark.parametrize("T", [1, 10, 100, 255])
def test_binary_tables_equal_the_restatement(cuda, T, d):
    from dal.forest import Forest

    F = Forest.synthetic(T, 3 if d == 5 else 4, d, seed=T + d)
    rules = {_check_case(cuda, n, d, F, seed=n + T) for n in SIZES}
    # the host rule picks the kernel: every shape runs blocked and row-major but
    # 256 features x 255 trees, whose forest and tile exceed the LDS bound
    assert rules == ({0} if (T, d) == (255, 256) else {64})


@pytest.mark.parametrize("d", [5, 30, 256])
@pytest.mark.parametrize("T", [7, 255])
@pytest.mark.parametrize("C", [3, 5, 32])
def test_multiclass_tables_equal_the_restatement(cuda, C, T, d):
    from dal.forest import Forest

    F = Forest.synthetic(T, 3 if d == 5 else 4, d, seed=C + T + d, n_classes=C)
    rules = {_check_case(cuda, n, d, F, seed=n + C) for n in SIZES}
    assert rules == ({0} if (T, d) == (255, 256) else {64})


def test_two_class_forest_of_the_multiclass_builder_and_many_trees(cuda):
    """n_classes == 2 takes the vote-count table whatever built the forest; a
    forest past the blocked rule's tree limit (T > 1020) takes the row-major
    kernel up to DAL_LAL_MAX_TREES."""
    from dal.forest import Forest

    F = Forest.synthetic(9, 4, 30, seed=2, n_classes=2)
    assert _check_case(cuda, 300, 30, F, seed=5) == 64
    F = Forest.synthetic(4095, 1, 5, seed=3)
    assert _check_case(cuda, 130, 5, F, seed=6) == 0


def test_label_and_leaf_bytes_outside_the_classes_are_counted_nowhere(cuda):
    from dal.forest import Forest

    for C, T in ((2, 10), (5, 7)):
        n, d = 333, 30
        F = Forest.synthetic(T, 4, d, seed=4, n_classes=C)
        X = _pool(n, d, F, seed=9)
        case = _Case(cuda, X, F)
        assert case.forms() == ("rows", "blocked")
        # all labels one class
        for c in (0, C - 1):
            y = np.full(n, c, np.uint8)
            want = np.array(R.joint_table(F, X, y), dtype=np.int64)
            for form in case.forms():
                assert np.array_equal(case.table(form, _dev(cuda, y)), want), (C, c, form)
        # label bytes >= C (the Python layer refuses them; the kernel counts them nowhere)
        y = np.random.default_rng(1).integers(0, C, n).astype(np.uint8)
        y[::5] = C
        y[3::11] = 255
        want = np.array(R.joint_table(F, X, y), dtype=np.int64)
        assert 0 < int(want.sum()) < n
        for form in case.forms():
            assert np.array_equal(case.table(form, _dev(cuda, y)), want), (C, form)
        # a leaf byte >= C: the rows reaching it are counted nowhere
        leaf = F.leaf.copy()
        leaf[0, :4] = C
        leaf[T - 1, -1] = 200
        G = Forest(inner=F.inner.copy(), leaf=leaf, depth=F.depth, n_classes=C)
        y = np.random.default_rng(2).integers(0, C, n).astype(np.uint8)
        want = np.array(R.joint_table(G, X, y), dtype=np.int64)
        assert 0 < int(want.sum()) < n
        bad = _Case(cuda, X, G)
        for form in bad.forms():
            assert np.array_equal(bad.table(form, _dev(cuda, y)), want), (C, form)


def test_flags_select_the_rows(cuda):
    from dal.forest import Forest

    n, d = 1000, 30
    for C, T in ((2, 100), (3, 7)):
        F = Forest.synthetic(T, 4, d, seed=8, n_classes=C)
        X = _pool(n, d, F, seed=3)
        y = np.random.default_rng(4).integers(0, C, n).astype(np.uint8)
        case = _Case(cuda, X, F)
        sparse = np.where(np.arange(n) % 7 == 0, 1, 2).astype(np.uint8)   # candidates, the rest excluded
        sparse[::14] = 3                                                  # both bits: still a candidate
        for flags in (sparse, np.zeros(n, np.uint8), np.ones(n, np.uint8), None):
            want = np.array(R.joint_table(F, X, y, flags=flags), dtype=np.int64)
            for form in case.forms():
                got = case.table(form, _dev(cuda, y), None if flags is None else _dev(cuda, flags))
                assert np.array_equal(got, want), (C, form)
        assert int(np.array(R.joint_table(F, X, y, flags=sparse)).sum()) == 143


def test_calls_accumulate_and_row_ranges_compose(cuda):
    import torch

    from dal.forest import Forest

    n, d = 1000, 30
    for C, T in ((2, 10), (5, 7)):
        F = Forest.synthetic(T, 4, d, seed=12, n_classes=C)
        X = _pool(n, d, F, seed=13)
        y = np.random.default_rng(14).integers(0, C, n).astype(np.uint8)
        case = _Case(cuda, X, F)
        yd = _dev(cuda, y)
        want = np.array(R.joint_table(F, X, y), dtype=np.int64).reshape(-1)
        for form in case.forms():
            h = case.run(form, yd)
            assert np.array_equal(h.cpu().numpy(), want)
            case.run(form, yd, hist=h)                       # a second call doubles every cell
            assert np.array_equal(h.cpu().numpy(), 2 * want), form
            for cut in (128, 640):                           # two row ranges into one table, two splits
                h = case.run(form, yd, n=cut)
                case.run(form, yd, hist=h, row0=cut)
                assert np.array_equal(h.cpu().numpy(), want), (form, cut)
            h = torch.zeros_like(h)
            case.run(form, yd, hist=h, n=0)                  # n == 0 launches nothing
            assert int(h.sum()) == 0


# ------------------------------------------------------------ end to end --
@pytest.mark.parametrize("name", ["checkerboard2x2.npz", "checkerboard4x4.npz"])
def test_evaluate_on_the_checkerboard_pools(cuda, name):
    from dal import metrics
    from dal import random_forest as rf
    from dal.engine import PoolState

    g = load_golden(name)
    X, y = g["X"], g["y"]
    F = rf.train_classifier(X[:200], y[:200], num_trees=10, seed=3, device=cuda)
    Xt, yt = X[200:], y[200:]
    want = R.evaluate(F, Xt, yt, BINARY)
    assert want["TP"] and want["TN"] and 0.0 < want["auc"] < 1.0  # (both classes, on both sides)
    got = metrics.evaluate(F, Xt, yt, BINARY, device=cuda)          # an array: the row-major kernel
    assert R.same(got, want)
    st = PoolState(Xt, device=cuda)
    got = metrics.evaluate(F, st, yt, BINARY)                       # a PoolState: its blocked copy, the prepared forest
    assert R.same(got, want) and st._xb is not None
    labels, votes = rf.predict(F, st)
    assert got["TP"] + got["TN"] == int((labels.cpu().numpy() == yt).sum())
    table = np.array(R.joint_table(F, Xt, yt))
    assert np.array_equal(np.bincount(votes.cpu().numpy(), minlength=11), table.sum(axis=1))
    flags = (np.arange(Xt.shape[0]) % 3 == 0).astype(np.uint8)
    assert R.same(metrics.evaluate(F, st, yt, BINARY, flags=flags), R.evaluate(F, Xt, yt, BINARY, flags=flags))
    with pytest.raises(ValueError, match="class ids"):
        metrics.evaluate(F, st, np.where(yt == 1, 2, 0))


def test_evaluate_multiclass(cuda):
    from dal import metrics
    from dal import random_forest as rf
    from dal.engine import PoolState
    from dal.forest import Forest

    n, d, C = 700, 30, 5
    F = Forest.synthetic(15, 4, d, seed=21, n_classes=C)
    X = _pool(n, d, F, seed=22)
    y = np.random.default_rng(23).integers(0, C, n)
    st = PoolState(X, device=cuda)
    got = metrics.evaluate(F, st, y, ("accuracy", "confusion"))
    assert R.same(got, R.evaluate(F, X, y, ("accuracy", "confusion")))
    pred, _ = rf.predict(F, st)
    assert int(np.trace(got["confusion"])) == int((pred.cpu().numpy() == y).sum())
    F.classes_ = np.array([3, 5, 8, 13, 21])                       # labels, mapped to ids before upload
    assert R.same(metrics.evaluate(F, st, F.classes_[y], ("accuracy", "confusion")), got)
    with pytest.raises(ValueError, match="two classes"):
        metrics.evaluate(F, st, y, ("auc",))


# -------------------------------------------------------------------- MSE --
@pytest.mark.parametrize("f64", [False, True])
def test_mean_squared_error_bits(cuda, f64):
    from dal import metrics
    from dal import random_forest as rf
    from dal.forest import RegressionForest

    d = 12
    M = RegressionForest.synthetic(20, 4, d, seed=5)                # leaves eleven decades apart
    for n in SIZES:
        rng = np.random.default_rng(n)
        X = rng.random((n, d)) if f64 else rng.random((n, d), dtype=np.float32)
        pred = rf.predict_regression(M, X, device=cuda).cpu().numpy()
        y = pred + np.where(rng.random(n) < 0.3, 0.0, rng.standard_normal(n) * 10.0 ** rng.integers(-6, 5, n))
        assert n < 63 or (y == pred).any()                          # exact zeros among the residuals
        got = metrics.mean_squared_error(M, X, y, device=cuda)
        want = R.mse(pred, y)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (n, got, want)


def test_sq_error_cells_and_refusals(cuda):
    import torch

    from dal import metrics

    def cells(pred, y):
        return metrics.sq_error_cells(torch.tensor(pred, dtype=torch.float64, device=cuda),
                                      torch.tensor(y, dtype=torch.float64, device=cuda))

    rng = np.random.default_rng(31)
    y = rng.standard_normal(5000)
    e = np.where(np.arange(5000) % 2 == 0, 1e5, 1e-6) * rng.uniform(0.5, 1.0, 5000)   # eleven decades apart
    e[::9] = 0.0
    pred = y - e
    words, q = cells(pred, y)
    s = R.squared_errors(pred, y)
    low, top = R.sum_format(s)
    assert (q, len(words)) == metrics.sq_error_limbs(low, top) and len(words) > 1
    from fractions import Fraction

    total = sum(int(w) << (31 * j) for j, w in enumerate(words))
    assert Fraction(total) * Fraction(2) ** q == sum((Fraction(float(v)) for v in s), Fraction(0))
    assert metrics.mse_from_cells(words, q, 5000) == R.mse(pred, y)
    # the same words for another row order
    perm = rng.permutation(5000)
    w2, q2 = cells(pred[perm], y[perm])
    assert q2 == q and np.array_equal(w2, words)
    # every residual zero, and no rows
    words, q = cells(np.arange(7.0), np.arange(7.0))
    assert q == 0 and list(words) == [0] and metrics.mse_from_cells(words, q, 7) == 0.0
    words, q = cells([], [])
    assert list(words) == [0] and math.isnan(metrics.mse_from_cells(words, q, 0))
    # subnormal squares; 242 bits between the highest and the lowest set bit: 8 limbs
    for pred, y in (([0.0] * 3, [1e-160, 3e-162, 2.0 ** -537]), ([0.0] * 3, [2.0 ** 60, 1.0, 3 * 2.0 ** -60])):
        words, q = cells(pred, y)
        assert metrics.mse_from_cells(words, q, 3) == R.mse(pred, y)
    assert len(words) == 8
    with pytest.raises(ValueError, match="span 281 bits"):
        cells([0.0, 0.0], [2.0 ** 70, 3 * 2.0 ** -70])
    for bad in (1e200, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="not finite"):
            cells([0.0, 1.0], [bad, 2.0])


# ------------------------------------------------------------------- loop --
def test_gpu_loop_measures_equal_the_restatement(cuda):
    from dal import loop

    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"][:400], g["y"][:400]
    Xt, yt = g["X"][400:], g["y"][400:]
    names = ("accuracy", "auc", "TP", "TN", "FP", "FN")
    base = loop.run_loop(X, y, Xt, yt, window_size=10, max_iterations=6, device=cuda, trainer="gpu")
    got = loop.run_loop(X, y, Xt, yt, window_size=10, max_iterations=6, device=cuda, trainer="gpu", measures=names)
    assert base.metrics == [] and len(got.metrics) == 6
    assert got.log == base.log and got.accuracy == base.accuracy  # the measures change nothing else
    forests = []

    def trainer(Xl, yl, T, seed):
        model = loop.train_forest(Xl, yl, T, seed, trainer="gpu", device=cuda)
        forests.append(model.forest)
        return model

    again = loop.run_loop(X, y, Xt, yt, window_size=10, max_iterations=6, device=cuda, trainer=trainer,
                          measures=names)
    assert again.log == got.log and len(forests) == 6
    for it, (m, m2, F, acc) in enumerate(zip(got.metrics, again.metrics, forests, got.accuracy)):
        want = R.evaluate(F, Xt, yt, names)
        assert R.same(m, want) and R.same(m2, want), it
        assert m["TP"] + m["TN"] == round(acc * 6)               # the loop's percent of 600 rows
