"""Soft-vote BALD, host side: the forest's leaf entropy words against the
restatement (tests/bald_reference.py), the definition against the directly
computed mean KL divergence, why the strategy exists, the two LDS budgets,
every host-side status of dal_forest_score_soft_bald and the argument checks.
CPU only (no kernel launches)."""
import ctypes

import numpy as np
import pytest

import bald_cases as BC
import bald_reference as B
import soft_reference as R
from dal import _lib
from dal.forest import ProbabilityForest, leaf_entropy_words, quantize_distribution


def test_shift_and_symbol():
    assert _lib.DAL_SOFT_ENTROPY_SHIFT == B.SHIFT == 29
    lib = _lib.load()
    assert lib.dal_abi_version() == 10  # a new symbol only
    assert hasattr(lib, "dal_forest_score_soft_bald")


@pytest.mark.parametrize("name", ["scalar_ragged", "wide_resident", "widest_one_hot", "between_budgets"])
def test_leaf_words_equal_the_restatement(name):
    """A scikit-learn fit (odd C, W = 32) and synthetic forests."""
    _, F, _, _, _ = BC.case(name)
    h = F.leaf_h
    assert h.dtype == np.uint32 and h.shape == (F.n_leaves,)
    assert F.leaf_h is h  # computed once
    ref = B.leaf_words(F)
    assert all(0 <= w < 1 << 32 for w in ref)
    assert h.tolist() == ref
    F.check()


def test_one_hot_and_uniform_leaves():
    one_hot = np.zeros((1, 5))
    one_hot[0, 3] = 2.5
    assert leaf_entropy_words(quantize_distribution(one_hot)).tolist() == [0]
    uniform = quantize_distribution(np.ones((1, 32)))
    assert uniform.tolist() == [[1 << 26] * 32]
    assert leaf_entropy_words(uniform).tolist() == [5 << 29] and 5 << 29 < 1 << 32
    assert B.leaf_word([1 << 26] * 32) == 5 << 29 and B.leaf_word([0, 0, R.ONE]) == 0
    # row 0 of the one-hot case reaches only one-hot leaves
    X, F, S, HS, _ = BC.case("widest_one_hot")
    assert HS[0] == 0 and (F.leaf_h == 0).sum() >= 1
    assert B.scores(S[:1], HS[:1], 255)[0] == 0.0 and not np.signbit(B.scores(S[:1], HS[:1], 255)[0])
    # the largest sum a row can have stays exact in fp64
    assert 255 * (5 << 29) < 1 << 41


def test_check_verifies_the_word_table():
    F = ProbabilityForest.synthetic(5, 3, 8, 4, seed=2)
    F.check()
    F._dev["leaf_h"] = F.leaf_h[:-1]
    with pytest.raises(ValueError, match="leaf_h"):
        F.check()
    with pytest.raises(ValueError, match="leaf_h"):
        F.device_leaf_h("cuda:0")  # before any upload
    F._dev["leaf_h"] = leaf_entropy_words(F.leaf_q).astype(np.int64)
    with pytest.raises(ValueError, match="leaf_h"):
        F.check()


def test_the_definition_is_the_mean_kl_divergence():
    """max(e - Hs / (T 2^29), 0) against (1/T) sum_t KL(p_t || pbar) in fp64:
    the bound is the 2^-30 word rounding of the mean plus fp64 noise."""
    X, F, S, HS, _ = BC.case("scalar_ragged")
    assert BC.CASES["scalar_ragged"] == (1037, 30, 10, 4, 3)
    got, ref = B.scores(S, HS, 10), B.mean_kl(F, X)
    gap = np.abs(got - ref).max()
    print(f"max |bald - mean KL| = {gap:.3e} = {gap * 2.0 ** 29:.3f} x 2^-29 (bound 1 x 2^-29)")
    assert gap <= 2.0 ** -29
    assert (got >= 0).all() and not np.signbit(got).any() and got.max() > 0.05
    impure = np.mean(F.leaf_h != 0)
    print(f"impure leaves: {impure:.2f}")
    assert impure > 0.25  # a depth-limited forest: the leaf entropies matter


def test_bald_selects_other_rows_than_the_entropy():
    """What the strategy is for: the top-10 of the disagreement and of the
    consensus entropy differ."""
    X, F, S, HS, _ = BC.case("scalar_ragged")
    idx = np.arange(len(S))
    top_b, _ = R.topk(B.scores(S, HS, 10), idx, 10, False)
    top_e, _ = R.topk(R.scores(S, 10, "entropy"), idx, 10, False)
    print(f"rows in both top-10: {np.intersect1d(top_b, top_e).size}")
    assert set(top_b.tolist()) != set(top_e.tolist())


def test_single_tree_scores_are_rounding_only():
    """T = 1: H(pbar) = H(p_1), so every score lies in [+0.0, 2^-29] and the
    clamp is at work."""
    X, F, S, HS, _ = BC.case("single_tree")
    raw = np.array([float(e) - float(h) / float(1 << 29) for e, h in zip(R.scores(S, 1, "entropy"), HS)])
    sc = B.scores(S, HS, 1)
    assert (raw < 0).any() and (sc >= 0).all() and sc.max() <= 2.0 ** -29 and not np.signbit(sc).any()


def test_a_forest_between_the_two_budgets():
    """The entropy kernel keeps the forest of "between_budgets" in LDS and the
    BALD kernel does not (even C: the leaf row grows from 2 to 4 words); the
    other cases fall on the side they are listed for."""
    n, d, T, depth, C = BC.CASES["between_budgets"]
    F = BC.case("between_budgets")[1]
    assert F.n_leaves == T << depth
    assert B.forest_lds_bytes(T, depth, F.n_leaves, C, False) == 10 * (255 * 8 + 256 * 4) + 2560 * 2 * 4 == 51120
    assert B.forest_lds_bytes(T, depth, F.n_leaves, C, True) == 10 * (255 * 8 + 256 * 4) + 2560 * 4 * 4 == 71600
    assert B.resident(F, False) and not B.resident(F, True)
    for name in BC.CASES:
        F = BC.case(name)[1]
        # (the 2,040 32-class leaves of "widest_one_hot" exceed the budget of either kernel)
        want = name not in ("forest_global", "between_budgets", "widest_one_hot")
        assert B.resident(F, True) == want, name
        assert B.resident(F, False) == (want or name == "between_budgets"), name
    # odd C: the word takes the padding slot, the row does not grow
    assert B.forest_lds_bytes(10, 4, 100, 3, True) == B.forest_lds_bytes(10, 4, 100, 3, False)
    assert B.forest_lds_bytes(10, 4, 100, 2, True) - B.forest_lds_bytes(10, 4, 100, 2, False) == 100 * 8


def test_abi_statuses_without_gpu():
    lib = _lib.load()
    limit = lib.dal_forest_soft_max_depth()
    p = ctypes.c_void_p(256)
    ARG, SHAPE, UNSUPPORTED = -1, -2, -3

    def score(x=p, n=10, d=4, x_stride=4, inner=p, leaf_id=p, leaf_q=p, leaf_h=p, L=20, T=10, depth=4, C=3,
              flags=None, order=1, sums=p, pred=p, hsum=p, entropy=p, scores=p, keys=p):
        return lib.dal_forest_score_soft_bald(x, n, d, x_stride, inner, leaf_id, leaf_q, leaf_h, L, T, depth, C, flags,
                                              order, sums, pred, hsum, entropy, scores, keys, None)

    for name in ("x", "inner", "leaf_id", "leaf_q", "leaf_h", "scores", "keys"):
        assert score(**{name: None}) == ARG, name
    assert score(order=2) == ARG and score(order=-1) == ARG
    assert score(x_stride=3) == SHAPE and score(d=30, x_stride=29) == SHAPE and score(d=30, x_stride=0) == SHAPE
    assert score(n=-1) == SHAPE and score(d=0, x_stride=0) == SHAPE and score(L=0) == SHAPE
    assert score(L=(1 << 26) + 1) == SHAPE
    assert score(T=256) == UNSUPPORTED and score(T=0) == UNSUPPORTED
    assert score(C=33) == UNSUPPORTED and score(C=1) == UNSUPPORTED
    assert score(depth=limit + 1) == UNSUPPORTED and score(depth=0) == UNSUPPORTED
    # the documented order: ARG before SHAPE before UNSUPPORTED
    assert score(leaf_h=None, x_stride=3) == ARG
    assert score(leaf_h=None, x_stride=3, T=256) == ARG
    assert score(x_stride=3, T=256) == SHAPE and score(x_stride=3, C=33, depth=limit + 1) == SHAPE
    # nothing to score: no launch; sums, pred, hsum and entropy are optional; the limits themselves pass
    assert score(n=0) == 0 and score(n=0, sums=None, pred=None, hsum=None, entropy=None) == 0
    assert score(n=0, order=0) == 0
    assert score(n=0, T=255, C=32, depth=limit) == 0 and score(n=0, T=1, C=2, depth=1, d=1, x_stride=1) == 0
    assert score(n=0, x_stride=7) == 0  # any stride >= d


def test_argument_checks():
    from dal import luts, parallel
    from dal import uncertainty_sampling as us
    from dal.engine import soft_step
    from dal.loop import run_loop

    X, F, _, _, _ = BC.case("scalar_ragged")
    hard = F.hard()  # (refused before any upload: without a GPU an upload raises something else)
    unl = np.arange(10, 1037)
    with pytest.raises(ValueError, match="ProbabilityForest"):
        us.select(X, unl, hard, 5, strategy="bald")
    with pytest.raises(ValueError, match="ProbabilityForest"):
        us.select_batch(X, unl, np.arange(10), hard, 5, strategy="bald")
    with pytest.raises(ValueError, match="strategy must be one of"):
        us.select(X, unl, F, 5, strategy="disagreement")
    with pytest.raises(ValueError, match="ProbabilityForest"):
        parallel._soft_forest(hard, "us", "bald")
    assert parallel._soft_forest(F, "us", "bald") is True
    with pytest.raises(ValueError, match="bald"):
        soft_step(None, unl, F, 5, strategy="vote_entropy")
    # the loop: soft votes by definition, so the GPU trainer (no leaf distributions) is refused
    rng = np.random.default_rng(3)
    Xl = rng.random((240, 6)).astype(np.float32)
    y = (Xl[:, 0] * 3).astype(int).clip(0, 2)
    with pytest.raises(ValueError, match="trainer='gpu'"):
        run_loop(Xl, y, strategy="bald", trainer="gpu", num_classes=3, max_iterations=1)
    with pytest.raises(ValueError, match="trainer='gpu'"):
        run_loop(Xl, y, strategy="bald", soft_votes=True, num_classes=3, max_iterations=1)
    with pytest.raises(ValueError, match="density_over"):
        run_loop(Xl, y, strategy="bald", trainer="sklearn", density_over="unlabeled", max_iterations=1)
    # the batch weight: the entropy rule, score / log2(C) capped at 1
    sc = np.array([0.0, 0.25, 1.0, np.log2(3.0), 1.6])
    w = luts.batch_weights_multiclass("bald", sc, 3)
    assert w.tobytes() == luts.batch_weights_multiclass("entropy", sc, 3).tobytes()
    assert w.tobytes() == np.minimum(sc / (np.log(3) / np.log(2)), 1.0).tobytes() and w[-1] == 1.0 and w[0] == 0.0
    import torch

    wt = luts.batch_weights_multiclass("bald", torch.from_numpy(sc), 3)
    assert wt.numpy().tobytes() == w.tobytes()


def test_run_loop_bald_with_the_restatement():
    """select_fn replaces the step: strategy "bald" reaches it with its name,
    and soft_votes=True is redundant."""
    from dal.loop import run_loop

    rng = np.random.default_rng(3)
    X = rng.random((240, 6)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2)
    seen = []

    def select_fn(strategy, pool, unlabeled, model, k):
        seen.append(strategy)
        F = ProbabilityForest.from_sklearn(model)
        Xu = pool[unlabeled]
        return R.topk(B.scores(R.sums(F, Xu), B.hsums(F, Xu), F.n_trees), unlabeled, k, False)[0]

    kw = dict(strategy="bald", window_size=20, n_estimators=10, max_iterations=2, seed=4, trainer="sklearn",
              select_fn=select_fn)
    a, b = run_loop(X, y, **kw), run_loop(X, y, soft_votes=True, **kw)
    assert seen == ["bald"] * 4 and len(a.labeled_history) == 2
    for u, v in zip(a.labeled_history, b.labeled_history):
        assert np.array_equal(u, v)
    assert np.unique(np.concatenate(a.labeled_history)).size == 40
