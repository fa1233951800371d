"""Random-forest models in the device SoA layout used by ``dal_forest_score``.

Reference: the forest is ``RandomForest.trainClassifier(..., numTrees=T,
featureSubsetStrategy="auto", impurity='gini')`` (uncertainty_sampling.py:71-76,
density_weighting.py:119-124; MLlib default maxDepth=4) and the hot path walks
``model._java_model.trees()`` calling ``DecisionTreeModel(tree).predict``
(uncertainty_sampling.py:89-90).  MLlib 2.1 ``Node.predict`` sends a row left
when ``x[feature] <= threshold`` (continuous split) and a leaf returns its
class label.

Layout (per tree, complete binary heap of the forest's maximum depth D):
  inner[t][h] = (feature:int32, threshold:fp32 bits)   h < 2^D - 1
  leaf[t][l]  = class in {0,1}                          l < 2^D
                (a multiclass forest, n_classes = C > 2: class id in {0..C-1})
Shallower leaves are padded with always-left splits (threshold = +inf) whose
whole subtree carries the leaf's class, so every root-to-leaf walk is exactly
D steps (wave-uniform trip count on the GPU).  Thresholds are rounded toward
-inf to fp32: for every fp32 x,  x <= t32  <=>  (double)x <= t64, so votes are
bit-exact against scikit-learn (fp32 X, fp64 thresholds) and against MLlib's
fp64 comparison FOR fp32-REPRESENTABLE FEATURE VALUES (the pool is fp32 here;
text features that are not fp32-representable are rounded on ingest, and a
value within that rounding of an fp64 MLlib threshold can fall on the other
side -- parity unpinned for such data: no reference-held model covers it).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from ._lib import (DAL_MAX_TREE_DEPTH, DAL_MC_MAX_CLASSES, DAL_REG_MAX_DEPTH, DAL_SOFT_ENTROPY_SHIFT,
                   DAL_SOFT_MAX_CLASSES, DAL_SOFT_MAX_DEPTH, DAL_SOFT_MAX_TREES, DAL_SOFT_ONE)

_POS_INF_BITS = np.array([np.inf], dtype=np.float32).view(np.int32)[0]


def threshold_to_f32(t64: np.ndarray) -> np.ndarray:
    """Largest fp32 <= t64 (round toward -inf)."""
    t64 = np.asarray(t64, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = t64.astype(np.float32)
    over = f.astype(np.float64) > t64
    f[over] = np.nextafter(f[over], np.float32(-np.inf))
    return f


@dataclass
class Forest:
    """A forest of hard-voting trees: binary (n_classes = 2, votes for class
    1) or multiclass (leaf bytes are class ids in {0..n_classes-1};
    ``classes_`` optionally holds the label of each class id)."""

    inner: np.ndarray  # int32 [T, 2^D - 1, 2]
    leaf: np.ndarray  # uint8 [T, 2^D]
    depth: int
    _dev: dict = field(default_factory=dict, repr=False)
    n_classes: int = 2
    classes_: np.ndarray = None

    @property
    def n_trees(self) -> int:
        return int(self.inner.shape[0])

    def check_features(self, d: int):
        """Raise unless every inner node tests a feature in [0, d): the score
        kernels index the pool row (or the blocked copy's feature list) with it."""
        if "range" not in self._dev:
            f = self.inner[..., 0]
            self._dev["range"] = (int(f.min()), int(f.max())) if f.size else (0, 0)
        lo, hi = self._dev["range"]
        if lo < 0 or hi >= d:
            raise ValueError(f"forest tests feature {lo if lo < 0 else hi}, outside the pool's {d} features")

    def check_classes(self):
        """Raise unless 2 <= n_classes <= DAL_MC_MAX_CLASSES and every leaf is
        a class id below n_classes: the multiclass score kernel counts such a
        leaf for no class."""
        C = int(self.n_classes)
        if not 2 <= C <= DAL_MC_MAX_CLASSES:
            raise ValueError(f"n_classes must lie in [2, {DAL_MC_MAX_CLASSES}], not {C}")
        if "leaf_max" not in self._dev:
            self._dev["leaf_max"] = int(self.leaf.max()) if self.leaf.size else 0
        if self._dev["leaf_max"] >= C:
            raise ValueError(f"forest has a leaf of class {self._dev['leaf_max']}, outside its {C} classes")

    def device(self, device):
        """(inner, leaf) as device tensors, uploaded once per device."""
        import torch

        key = str(device)
        if key not in self._dev:
            self._dev[key] = (
                torch.from_numpy(np.ascontiguousarray(self.inner)).to(device),
                torch.from_numpy(np.ascontiguousarray(self.leaf)).to(device),
            )
        return self._dev[key]

    def blocked_prep(self, device, d: int):
        """The forest prepared for the blocked score kernel over d features
        (dal_forest_prepare, ABI v10: feature list, remapped nodes, leaves), a
        16-B aligned uint8 device tensor built once per (device, d) on the
        current stream -- or None when the blocked path does not apply."""
        import torch

        from . import _lib

        key = ("prep", str(device), int(d))
        if key not in self._dev:
            lib = _lib.load()
            nb = int(lib.dal_forest_prep_bytes(int(d), self.n_trees, self.depth))
            buf = None
            if nb:
                self.check_features(int(d))
                inner, leaf = self.device(device)
                buf = torch.empty(nb, dtype=torch.uint8, device=device)  # (caching allocator: 512-B aligned)
                _lib.call("dal_forest_prepare", inner.data_ptr(), leaf.data_ptr(), self.n_trees, self.depth,
                          int(d), buf.data_ptr(), nb,
                          torch.cuda.current_stream(device).cuda_stream)
            self._dev[key] = buf
        return self._dev[key]

    # ------------------------------------------------------------ builders
    @classmethod
    def from_nodes(cls, feature, threshold, left, right, value, roots, n_classes: int = 2,
                   classes_=None) -> "Forest":
        """Flattened node arrays (global node ids): feature < 0 marks a leaf
        whose class is value[node]; internal nodes go to left[node] when
        x[feature] <= threshold[node] (fp64), else right[node].  n_classes 2:
        a leaf is class 1 when value[node] is non-zero; above 2 it is the
        class id value[node], which must lie in [0, n_classes)."""
        n_classes = int(n_classes)
        if not 2 <= n_classes <= DAL_MC_MAX_CLASSES:
            raise ValueError(f"n_classes must lie in [2, {DAL_MC_MAX_CLASSES}], not {n_classes}")
        feature = np.asarray(feature, dtype=np.int64)
        threshold = np.asarray(threshold, dtype=np.float64)
        left = np.asarray(left, dtype=np.int64)
        right = np.asarray(right, dtype=np.int64)
        value = np.asarray(value, dtype=np.int64)
        roots = np.asarray(roots, dtype=np.int64)
        if roots.size == 0:
            raise ValueError("forest has no trees")

        def tree_depth(root):
            best, stack = 0, [(int(root), 0)]
            while stack:
                nd, lv = stack.pop()
                if feature[nd] < 0:
                    best = max(best, lv)
                else:
                    stack.append((int(left[nd]), lv + 1))
                    stack.append((int(right[nd]), lv + 1))
            return best

        D = max(1, max(tree_depth(r) for r in roots))
        if D > DAL_MAX_TREE_DEPTH:
            raise ValueError(f"tree depth {D} exceeds DAL_MAX_TREE_DEPTH={DAL_MAX_TREE_DEPTH}")
        n_inner, n_leaf = (1 << D) - 1, 1 << D
        T = roots.size
        inner = np.zeros((T, n_inner, 2), dtype=np.int32)
        inner[:, :, 1] = _POS_INF_BITS
        leaf = np.zeros((T, n_leaf), dtype=np.uint8)
        thr32 = threshold_to_f32(threshold).view(np.int32)
        for t, root in enumerate(roots):
            stack = [(int(root), 0, 0)]  # (node, heap index, level)
            while stack:
                nd, h, lv = stack.pop()
                if feature[nd] < 0:
                    if n_classes == 2:
                        cls_ = np.uint8(1 if value[nd] else 0)
                    else:
                        if not 0 <= value[nd] < n_classes:
                            raise ValueError(f"leaf class {int(value[nd])} outside [0, {n_classes})")
                        cls_ = np.uint8(value[nd])
                    # pad the subtree below heap position h with the leaf class
                    span = 1 << (D - lv)
                    first_leaf = (h + 1) * span - 1 - n_inner
                    leaf[t, first_leaf:first_leaf + span] = cls_
                    continue  # padded inner nodes keep (0, +inf): always left
                inner[t, h, 0] = feature[nd]
                inner[t, h, 1] = thr32[nd]
                stack.append((int(left[nd]), 2 * h + 1, lv + 1))
                stack.append((int(right[nd]), 2 * h + 2, lv + 1))
        return cls(inner=inner, leaf=leaf, depth=D, n_classes=n_classes,
                   classes_=None if classes_ is None else np.asarray(classes_))

    @classmethod
    def from_sklearn(cls, rf, positive_label=1, multiclass: bool = False) -> "Forest":
        """From a fitted ``sklearn.ensemble.RandomForestClassifier``: each tree
        votes 1 when its leaf's majority class equals ``positive_label``.
        multiclass=True: a leaf is the arg-max index of ``tree_.value`` (the
        class id; ``classes_`` = rf.classes_ maps it back to the label, so
        labels need not be contiguous) and n_classes = len(rf.classes_),
        at least 2."""
        classes = np.asarray(rf.classes_)
        feat, thr, lft, rgt, val, roots = [], [], [], [], [], []
        base = 0
        for est in rf.estimators_:
            tr = est.tree_
            roots.append(base)
            cl = np.asarray(tr.children_left)
            cr = np.asarray(tr.children_right)
            is_leaf = cl < 0
            cid = np.argmax(tr.value[:, 0, :], axis=1)
            lab = classes[cid]
            feat.append(np.where(is_leaf, -1, tr.feature))
            thr.append(np.where(is_leaf, 0.0, tr.threshold))
            lft.append(np.where(is_leaf, -1, cl + base))
            rgt.append(np.where(is_leaf, -1, cr + base))
            val.append(np.where(is_leaf, cid.astype(np.int64) if multiclass
                                else (lab == positive_label).astype(np.int64), 0))
            base += tr.node_count
        nodes = (np.concatenate(feat), np.concatenate(thr), np.concatenate(lft), np.concatenate(rgt),
                 np.concatenate(val), np.array(roots))
        if multiclass:
            f = cls.from_nodes(*nodes, n_classes=max(2, classes.size), classes_=classes)
            f.check_classes()  # (a two-class forest keeps from_nodes' non-zero rule: ids 0 and 1)
            return f
        return cls.from_nodes(*nodes)

    @classmethod
    def from_mllib_debug_string(cls, text: str, n_classes=None) -> "Forest":
        """Parse MLlib's ``RandomForestModel.toDebugString()`` (Spark 2.1
        ``Node.subtreeToString``): ``Tree k:`` headers, ``If (feature f <= t)`` /
        ``Else (feature f > t)`` for continuous splits, ``Predict: c`` at leaves.
        Categorical splits are rejected (the reference uses
        ``categoricalFeaturesInfo={}``, uncertainty_sampling.py:73).
        n_classes None: the binary mapping (``Predict: 1.0`` is class 1, any
        other label class 0); else ``Predict: c`` is class id int(c) of a
        forest of n_classes (trainClassifier's numClasses)."""
        nodes = _parse_mllib_debug_string(text, lambda c: _mllib_class(c, n_classes))
        return cls._from_mllib_nodes(*nodes, n_classes)

    @classmethod
    def _from_mllib_nodes(cls, feat, thr, lft, rgt, val, roots, n_classes) -> "Forest":
        if n_classes is None:
            return cls.from_nodes(feat, thr, lft, rgt, val, roots)
        f = cls.from_nodes(feat, thr, lft, rgt, val, roots, n_classes=int(n_classes))
        f.check_classes()
        return f

    @classmethod
    def from_mllib_saved(cls, path: str, n_classes=None) -> "Forest":
        """Read an MLlib ``RandomForestModel.save(sc, path)`` directory: Parquet
        ``NodeData`` rows (treeId, nodeId, predict{predict, prob}, impurity,
        isLeaf, split{feature, threshold, featureType, categories}, leftNodeId,
        rightNodeId, infoGain) under ``path/data``; continuous splits only.
        n_classes: as from_mllib_debug_string."""
        nodes = _read_mllib_saved(path, lambda c: _mllib_class(c, n_classes))
        return cls._from_mllib_nodes(*nodes, n_classes)

    @classmethod
    def synthetic(cls, n_trees: int, depth: int, n_features: int, seed: int = 1,
                  dist: str = "uniform", n_classes: int = 2, skew: float = 0.0) -> "Forest":
        """BASELINE.json synthetic forest: T complete depth-``depth`` trees,
        feature ~ U{0..D-1}, threshold ~ U(0,1) (or N(0,1)) as fp32, leaf
        class ~ Bernoulli(0.5) -- the same draw order as the test oracle.
        n_classes = C: leaf class ~ U{0..C-1}; skew > 0: class 0 with
        probability ``skew`` instead (one more uniform draw per tree, after
        the classes).  The defaults make the same draws as before."""
        n_classes = int(n_classes)
        if not 2 <= n_classes <= DAL_MC_MAX_CLASSES:
            raise ValueError(f"n_classes must lie in [2, {DAL_MC_MAX_CLASSES}], not {n_classes}")
        rng = np.random.default_rng(seed)
        n_inner, n_leaf = (1 << depth) - 1, 1 << depth
        inner = np.zeros((n_trees, n_inner, 2), dtype=np.int32)
        leaf = np.zeros((n_trees, n_leaf), dtype=np.uint8)
        for t in range(n_trees):
            f = rng.integers(0, n_features, size=n_inner)
            if dist == "uniform":
                th = rng.random(n_inner).astype(np.float32)
            else:
                th = rng.standard_normal(n_inner).astype(np.float32)
            lv = rng.integers(0, n_classes, size=n_leaf)
            if skew > 0.0:
                lv = np.where(rng.random(n_leaf) < skew, 0, lv)
            inner[t, :, 0] = f
            inner[t, :, 1] = th.view(np.int32)
            leaf[t] = lv
        return cls(inner=inner, leaf=leaf, depth=depth, n_classes=n_classes)


def _mllib_class(label: float, n_classes) -> int:
    """A leaf's class from MLlib's ``Predict: c``: the binary mapping
    (c == 1.0) when n_classes is None, else the class id int(c)."""
    if n_classes is None:
        return 1 if label == 1.0 else 0
    if label != int(label) or not 0 <= int(label) < int(n_classes):
        raise ValueError(f"leaf label {label} is not a class id in [0, {int(n_classes)})")
    return int(label)


def _parse_mllib_debug_string(text: str, leaf_value):
    """The node arrays (feature, threshold, left, right, value, roots) of
    MLlib's ``toDebugString()`` text; ``leaf_value`` maps a leaf's ``Predict:``
    double to the value kept (a class id, or the double itself)."""
    import re

    lines = [ln.strip() for ln in text.splitlines() if ln.strip()]
    trees, cur = [], None
    for ln in lines:
        if re.match(r"^Tree \d+:$", ln):
            cur = []
            trees.append(cur)
        elif cur is not None and (ln.startswith("If ") or ln.startswith("Else ")
                                  or ln.startswith("Predict:")):
            cur.append(ln)
    if not trees:
        raise ValueError("no 'Tree k:' sections found in the debug string")
    feat, thr, lft, rgt, val, roots = [], [], [], [], [], []
    if_re = re.compile(r"^If \(feature (\d+) <= ([^)]+)\)$")
    else_re = re.compile(r"^Else \(feature (\d+) > ([^)]+)\)$")

    def new_node():
        feat.append(-1)
        thr.append(0.0)
        lft.append(-1)
        rgt.append(-1)
        val.append(0)
        return len(feat) - 1

    for body in trees:
        pos = 0

        def parse():
            nonlocal pos
            ln = body[pos]
            pos += 1
            nd = new_node()
            if ln.startswith("Predict:"):
                val[nd] = leaf_value(float(ln.split(":", 1)[1]))
                return nd
            m = if_re.match(ln)
            if not m:
                raise ValueError(f"unsupported split line {ln!r} (only continuous splits)")
            feat[nd], thr[nd] = int(m.group(1)), float(m.group(2))
            lft[nd] = parse()
            m2 = else_re.match(body[pos])
            if not m2 or int(m2.group(1)) != feat[nd]:
                raise ValueError(f"malformed Else line {body[pos]!r}")
            pos += 1
            rgt[nd] = parse()
            return nd

        roots.append(parse())
    return feat, thr, lft, rgt, val, roots


def _read_mllib_saved(path: str, leaf_value):
    """The node arrays of an MLlib ``RandomForestModel.save`` directory
    (Parquet NodeData rows); ``leaf_value`` as _parse_mllib_debug_string."""
    import glob
    import os

    import pyarrow.parquet as pq

    data = os.path.join(path, "data") if os.path.isdir(os.path.join(path, "data")) else path
    files = sorted(glob.glob(os.path.join(data, "*.parquet")))
    if not files:
        raise ValueError(f"no parquet files under {data}")
    rows = []
    for f in files:
        rows.extend(pq.read_table(f).to_pylist())
    by_tree = {}
    for r in rows:
        by_tree.setdefault(int(r["treeId"]), {})[int(r["nodeId"])] = r
    feat, thr, lft, rgt, val, roots = [], [], [], [], [], []
    for t in sorted(by_tree):
        nodes = by_tree[t]
        gid = {nid: len(feat) + i for i, nid in enumerate(sorted(nodes))}
        for nid in sorted(nodes):
            r = nodes[nid]
            if r["isLeaf"]:
                feat.append(-1)
                thr.append(0.0)
                lft.append(-1)
                rgt.append(-1)
                val.append(leaf_value(float(r["predict"]["predict"])))
            else:
                sp = r["split"]
                if int(sp.get("featureType", 0)) != 0:
                    raise ValueError("categorical splits are not supported")
                feat.append(int(sp["feature"]))
                thr.append(float(sp["threshold"]))
                lft.append(gid[int(r["leftNodeId"])])
                rgt.append(gid[int(r["rightNodeId"])])
                val.append(0)
        roots.append(gid[min(nodes)])  # MLlib root node id = 1 (smallest)
    return feat, thr, lft, rgt, val, roots


@dataclass
class RegressionForest:
    """A regression forest, MLlib's ``RandomForest.trainRegressor`` model: the
    prediction is the mean of the trees' real-valued leaves
    (``RandomForestModel.predict``; the LAL model of
    lal_direct_mllib_implementation/classes/active_learner.py:319, :354-365).

    Layout: Forest's complete heap of the maximum depth D, padded the same way
    (a shallow leaf's subtree gets always-left splits, threshold +inf, and its
    value fills the subtree's leaves), with
      inner_feature    int32   [TR, 2^D - 1]
      inner_threshold  float64 [TR, 2^D - 1]   the model's value, NOT rounded
      leaf             float64 [TR, 2^D]
    The compare is fp64, ``row[feature] <= threshold`` goes left: LAL's rows
    (v/T, an SD, ...) are not fp32-representable, so Forest's fp32 thresholds
    rounded toward -inf would not keep MLlib's branches."""

    inner_feature: np.ndarray
    inner_threshold: np.ndarray
    leaf: np.ndarray
    depth: int
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def n_trees(self) -> int:
        return int(self.inner_feature.shape[0])

    def check_features(self, d: int):
        """Raise unless every inner node tests a feature in [0, d)."""
        if "range" not in self._dev:
            f = self.inner_feature
            self._dev["range"] = (int(f.min()), int(f.max())) if f.size else (0, 0)
        lo, hi = self._dev["range"]
        if lo < 0 or hi >= d:
            raise ValueError(f"forest tests feature {lo if lo < 0 else hi}, outside the rows' {d} features")

    def device(self, device):
        """(inner_feature, inner_threshold, leaf) as device tensors, uploaded
        once per device."""
        import torch

        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                   for a in (self.inner_feature, self.inner_threshold, self.leaf))
        return self._dev[key]

    # ------------------------------------------------------------ builders
    @classmethod
    def from_nodes(cls, feature, threshold, left, right, value, roots) -> "RegressionForest":
        """Flattened node arrays (global node ids), as Forest.from_nodes:
        feature < 0 marks a leaf whose prediction is value[node] (a double)."""
        feature = np.asarray(feature, dtype=np.int64)
        threshold = np.asarray(threshold, dtype=np.float64)
        left = np.asarray(left, dtype=np.int64)
        right = np.asarray(right, dtype=np.int64)
        value = np.asarray(value, dtype=np.float64)
        roots = np.asarray(roots, dtype=np.int64)
        if roots.size == 0:
            raise ValueError("forest has no trees")
        placed = []  # (tree, node, heap index, level)
        D = 1
        for t, root in enumerate(roots):
            stack = [(int(root), 0, 0)]
            while stack:
                nd, h, lv = stack.pop()
                placed.append((t, nd, h, lv))
                if feature[nd] < 0:
                    D = max(D, lv)
                    continue
                if lv >= DAL_REG_MAX_DEPTH:
                    raise ValueError(f"tree depth exceeds DAL_REG_MAX_DEPTH={DAL_REG_MAX_DEPTH}")
                stack.append((int(left[nd]), 2 * h + 1, lv + 1))
                stack.append((int(right[nd]), 2 * h + 2, lv + 1))
        n_inner, n_leaf = (1 << D) - 1, 1 << D
        T = roots.size
        inner_feature = np.zeros((T, n_inner), dtype=np.int32)
        inner_threshold = np.full((T, n_inner), np.inf, dtype=np.float64)
        leaf = np.zeros((T, n_leaf), dtype=np.float64)
        for t, nd, h, lv in placed:
            if feature[nd] < 0:
                span = 1 << (D - lv)  # the leaves below heap position h
                first_leaf = (h + 1) * span - 1 - n_inner
                leaf[t, first_leaf:first_leaf + span] = value[nd]
            else:
                inner_feature[t, h] = feature[nd]
                inner_threshold[t, h] = threshold[nd]
        return cls(inner_feature=inner_feature, inner_threshold=inner_threshold, leaf=leaf, depth=D)

    @classmethod
    def from_sklearn(cls, rf) -> "RegressionForest":
        """From a fitted ``sklearn.ensemble.RandomForestRegressor`` (single
        output): a leaf predicts ``tree_.value[node, 0, 0]``."""
        feat, thr, lft, rgt, val, roots = [], [], [], [], [], []
        base = 0
        for est in rf.estimators_:
            tr = est.tree_
            roots.append(base)
            cl = np.asarray(tr.children_left)
            cr = np.asarray(tr.children_right)
            is_leaf = cl < 0
            feat.append(np.where(is_leaf, -1, tr.feature))
            thr.append(np.where(is_leaf, 0.0, tr.threshold))
            lft.append(np.where(is_leaf, -1, cl + base))
            rgt.append(np.where(is_leaf, -1, cr + base))
            val.append(np.asarray(tr.value[:, 0, 0], dtype=np.float64))
            base += tr.node_count
        return cls.from_nodes(np.concatenate(feat), np.concatenate(thr), np.concatenate(lft), np.concatenate(rgt),
                              np.concatenate(val), np.array(roots))

    @classmethod
    def from_mllib_debug_string(cls, text: str) -> "RegressionForest":
        """Parse ``RandomForestModel.toDebugString()`` of a regression model:
        the classifier's grammar (Forest.from_mllib_debug_string) with
        ``Predict: <double>`` at the leaves; continuous splits only."""
        return cls.from_nodes(*_parse_mllib_debug_string(text, float))

    @classmethod
    def from_mllib_saved(cls, path: str) -> "RegressionForest":
        """Read an MLlib ``RandomForestModel.save(sc, path)`` directory of a
        regression model (what ``RandomForestModel.load`` reads,
        active_learner.py:361): NodeData ``predict.predict`` is the leaf's
        double."""
        return cls.from_nodes(*_read_mllib_saved(path, float))

    @classmethod
    def synthetic(cls, n_trees: int, depth: int, n_features: int, seed: int = 1,
                  dist: str = "uniform") -> "RegressionForest":
        """TR complete depth-``depth`` trees for tests and scripts: feature ~
        U{0..n_features-1}, threshold ~ U(0,1) ("uniform") or N(0,1) in fp64,
        leaf = +-10^e with e ~ U{-8..3} and a random sign -- magnitudes 11
        decades apart, so a sum taken in another order differs in its bits."""
        if not 1 <= depth <= DAL_REG_MAX_DEPTH:
            raise ValueError(f"depth must lie in [1, {DAL_REG_MAX_DEPTH}], not {depth}")
        rng = np.random.default_rng(seed)
        n_inner, n_leaf = (1 << depth) - 1, 1 << depth
        inner_feature = rng.integers(0, n_features, size=(n_trees, n_inner)).astype(np.int32)
        inner_threshold = rng.random((n_trees, n_inner)) if dist == "uniform" \
            else rng.standard_normal((n_trees, n_inner))
        e = rng.integers(-8, 4, size=(n_trees, n_leaf))
        sign = np.where(rng.random((n_trees, n_leaf)) < 0.5, -1.0, 1.0)
        leaf = sign * np.power(10.0, e.astype(np.float64))
        return cls(inner_feature=inner_feature, inner_threshold=inner_threshold.astype(np.float64),
                   leaf=leaf, depth=depth)


def quantize_distribution(distribution) -> np.ndarray:
    """Leaf class distributions [L, C] (weights or fractions, fp64) as the
    fixed-point leaf words of a ProbabilityForest: q = rint(p 2^31) as uint32,
    p = value / total in fp64, one division per class, total the fp64 sum of
    the row taken in class order; rounding to even, q <= 2^31.  A negative,
    NaN, infinite or all-zero row raises ValueError."""
    v = np.asarray(distribution, dtype=np.float64)
    if v.ndim != 2 or v.shape[0] < 1:
        raise ValueError("distribution must be a non-empty [leaves, classes] array")
    if not np.isfinite(v).all():
        raise ValueError("a leaf distribution holds a NaN or an infinite weight")
    if (v < 0).any():
        raise ValueError("a leaf distribution holds a negative weight")
    total = np.zeros(v.shape[0], dtype=np.float64)
    for c in range(v.shape[1]):  # class order: the restatement's sum
        total = total + v[:, c]
    if not (total > 0).all() or not np.isfinite(total).all():
        raise ValueError("a leaf distribution is all zero (or its sum overflows)")
    q = np.rint((v / total[:, None]) * float(DAL_SOFT_ONE))
    return q.astype(np.uint32)


def leaf_entropy_words(leaf_q) -> np.ndarray:
    """uint32 [L]: rint(H_l 2^29) of leaf words ``leaf_q`` [L, C] -- the
    entropy of the leaf's own fixed-point distribution, on Python floats in
    class order: e = 0.0; e = e + h(float(q) / 2.0**31), h(p) = (-p) log2(p),
    h(0) = +0.0; rounding half to even.  H_l <= log2(32) = 5, so a word is
    below 2^32 and a row's sum of at most 255 of them below 2^41."""
    q = np.asarray(leaf_q)
    if q.ndim != 2 or q.shape[1] > DAL_SOFT_MAX_CLASSES:
        raise ValueError(f"leaf_q must be [L, C] with C <= {DAL_SOFT_MAX_CLASSES}")
    one = 2.0 ** 31
    scale = float(1 << DAL_SOFT_ENTROPY_SHIFT)
    out = np.empty(q.shape[0], dtype=np.uint32)
    for l, row in enumerate(q.tolist()):
        e = 0.0
        for w in row:
            p = float(w) / one
            e = e + (0.0 if p == 0.0 else (-p) * math.log2(p))
        word = round(e * scale)  # (round(): half to even)
        if not 0 <= word < (1 << 32):
            raise ValueError("a leaf's entropy word leaves 32 bits: its words are no distribution")
        out[l] = word
    return out


@dataclass
class ProbabilityForest:
    """A forest of soft-voting trees: a leaf contributes its class distribution
    (scikit-learn's ``predict_proba``), not one class id.

    Layout (dal_forest_score_soft):
      inner    int32  [T, 2^D - 1, 2]  Forest's heap, (0, +inf) below a shallow leaf
      leaf_id  int32  [T, 2^D]         row of ``leaf_q`` of every heap leaf (a
                                       shallow leaf's id repeated over its subtree)
      leaf_q   uint32 [L, C]           rint(p 2^31) per class (quantize_distribution)
      leaf_h   uint32 [L]              rint(H_l 2^29), the entropy of the leaf's own
                                       words (leaf_entropy_words; computed on first
                                       use, dal_forest_score_soft_bald's fourth table)
    1 <= T <= 255, 2 <= C <= 32, D <= DAL_SOFT_MAX_DEPTH.  A row's class sums
    S_c = sum_t leaf_q[leaf_id[t, leaf_t(x)], c] are exact integers and the
    averaged probability is S_c / (T 2^31)."""

    inner: np.ndarray
    leaf_id: np.ndarray
    leaf_q: np.ndarray
    depth: int
    n_classes: int
    classes_: np.ndarray = None
    _dev: dict = field(default_factory=dict, repr=False)

    @property
    def n_trees(self) -> int:
        return int(self.inner.shape[0])

    @property
    def n_leaves(self) -> int:
        return int(self.leaf_q.shape[0])

    @property
    def denominator(self) -> int:
        """M = T 2^31: a row's class sums divided by it are its probabilities."""
        return self.n_trees * DAL_SOFT_ONE

    def check(self):
        """Raise unless the forest is within the kernel's limits and its tables
        are consistent (before any upload)."""
        _check_soft_limits(self.n_trees, int(self.n_classes), int(self.depth))
        T, D, C = self.n_trees, int(self.depth), int(self.n_classes)
        if self.inner.shape != (T, (1 << D) - 1, 2) or self.leaf_id.shape != (T, 1 << D):
            raise ValueError("inner must be [T, 2^D - 1, 2] and leaf_id [T, 2^D]")
        if self.leaf_q.ndim != 2 or self.leaf_q.shape[1] != C or self.leaf_q.shape[0] < 1:
            raise ValueError(f"leaf_q must be [L, {C}] with at least one leaf")
        if int(self.leaf_id.min()) < 0 or int(self.leaf_id.max()) >= self.n_leaves:
            raise ValueError(f"a leaf id lies outside the leaf table's {self.n_leaves} rows")
        if int(self.leaf_q.max()) > DAL_SOFT_ONE:
            raise ValueError("a leaf word exceeds 2^31")
        h = self._dev.get("leaf_h")
        if h is not None and (h.dtype != np.uint32 or h.shape != (self.n_leaves,)):
            raise ValueError(f"leaf_h must be uint32 [{self.n_leaves}], one entropy word per leaf")

    @property
    def leaf_h(self) -> np.ndarray:
        """uint32 [L]: every leaf's entropy word rint(H_l 2^29)
        (leaf_entropy_words of leaf_q), computed once on the host."""
        if "leaf_h" not in self._dev:
            self._dev["leaf_h"] = leaf_entropy_words(self.leaf_q)
        return self._dev["leaf_h"]

    def device_leaf_h(self, device):
        """leaf_h as a device tensor (its int32 bit pattern), uploaded once per
        device on first use; ``device()`` keeps returning its three tables."""
        import torch

        key = ("leaf_h", str(device))
        if key not in self._dev:
            h = self.leaf_h
            self.check()
            self._dev[key] = torch.from_numpy(np.ascontiguousarray(h, dtype=np.uint32).view(np.int32)).to(device)
        return self._dev[key]

    def check_features(self, d: int):
        """Raise unless every inner node tests a feature in [0, d)."""
        if "range" not in self._dev:
            f = self.inner[..., 0]
            self._dev["range"] = (int(f.min()), int(f.max())) if f.size else (0, 0)
        lo, hi = self._dev["range"]
        if lo < 0 or hi >= d:
            raise ValueError(f"forest tests feature {lo if lo < 0 else hi}, outside the pool's {d} features")

    def device(self, device):
        """(inner, leaf_id, leaf_q) as device tensors, uploaded once per device
        (leaf_q travels as its int32 bit pattern)."""
        import torch

        key = str(device)
        if key not in self._dev:
            self.check()
            self._dev[key] = (
                torch.from_numpy(np.ascontiguousarray(self.inner, dtype=np.int32)).to(device),
                torch.from_numpy(np.ascontiguousarray(self.leaf_id, dtype=np.int32)).to(device),
                torch.from_numpy(np.ascontiguousarray(self.leaf_q, dtype=np.uint32).view(np.int32)).to(device),
            )
        return self._dev[key]

    def hard(self) -> Forest:
        """The hard-voting Forest of arg-max leaves (the lowest class among
        equal largest words), over the same heap."""
        if "hard" not in self._dev:
            cls_ = np.argmax(self.leaf_q, axis=1).astype(np.uint8)
            self._dev["hard"] = Forest(inner=self.inner, leaf=cls_[self.leaf_id], depth=int(self.depth),
                                       n_classes=int(self.n_classes), classes_=self.classes_)
        return self._dev["hard"]

    # ------------------------------------------------------------ builders
    @classmethod
    def from_nodes(cls, feature, threshold, left, right, distribution, roots, n_classes: int,
                   classes_=None) -> "ProbabilityForest":
        """Flattened node arrays (global node ids), as Forest.from_nodes:
        feature < 0 marks a leaf whose class distribution is
        distribution[node] (C weights or fractions; rows of inner nodes are
        ignored).  Leaves are numbered tree by tree in the order a depth-first
        walk (left first) meets them."""
        n_classes = int(n_classes)
        feature = np.asarray(feature, dtype=np.int64)
        threshold = np.asarray(threshold, dtype=np.float64)
        left = np.asarray(left, dtype=np.int64)
        right = np.asarray(right, dtype=np.int64)
        roots = np.asarray(roots, dtype=np.int64)
        distribution = np.asarray(distribution, dtype=np.float64)
        if roots.size == 0:
            raise ValueError("forest has no trees")
        _check_soft_limits(int(roots.size), n_classes, 1)
        if distribution.ndim != 2 or distribution.shape != (feature.shape[0], n_classes):
            raise ValueError(f"distribution must be [nodes, {n_classes}]")
        placed = []  # (tree, node, heap index, level)
        D = 1
        for t, root in enumerate(roots):
            stack = [(int(root), 0, 0)]
            while stack:
                nd, h, lv = stack.pop()
                placed.append((t, nd, h, lv))
                if feature[nd] < 0:
                    D = max(D, lv)
                    continue
                if lv >= DAL_SOFT_MAX_DEPTH:
                    raise ValueError(f"tree depth exceeds DAL_SOFT_MAX_DEPTH={DAL_SOFT_MAX_DEPTH}")
                stack.append((int(right[nd]), 2 * h + 2, lv + 1))  # (popped after the left child)
                stack.append((int(left[nd]), 2 * h + 1, lv + 1))
        leaf_nodes = np.array([nd for _, nd, _, _ in placed if feature[nd] < 0], dtype=np.int64)
        leaf_q = quantize_distribution(distribution[leaf_nodes])
        n_inner, n_leaf = (1 << D) - 1, 1 << D
        T = roots.size
        inner = np.zeros((T, n_inner, 2), dtype=np.int32)
        inner[:, :, 1] = _POS_INF_BITS
        leaf_id = np.zeros((T, n_leaf), dtype=np.int32)
        thr32 = threshold_to_f32(threshold).view(np.int32)
        next_id = 0
        for t, nd, h, lv in placed:
            if feature[nd] < 0:
                span = 1 << (D - lv)  # the leaves below heap position h
                first_leaf = (h + 1) * span - 1 - n_inner
                leaf_id[t, first_leaf:first_leaf + span] = next_id
                next_id += 1
            else:
                inner[t, h, 0] = feature[nd]
                inner[t, h, 1] = thr32[nd]
        return cls(inner=inner, leaf_id=leaf_id, leaf_q=leaf_q, depth=D, n_classes=n_classes,
                   classes_=None if classes_ is None else np.asarray(classes_))

    @classmethod
    def from_sklearn(cls, rf) -> "ProbabilityForest":
        """From a fitted ``sklearn.ensemble.RandomForestClassifier``: every
        tree's ``tree_.value[:, 0, :]``, normalised per leaf; class id c is
        ``rf.classes_[c]`` (kept in ``classes_``).  A forest fitted on one
        label gets a second, empty class."""
        classes = np.asarray(rf.classes_)
        C = max(2, int(classes.size))
        feat, thr, lft, rgt, val, roots = [], [], [], [], [], []
        base = 0
        for est in rf.estimators_:
            tr = est.tree_
            roots.append(base)
            cl = np.asarray(tr.children_left)
            cr = np.asarray(tr.children_right)
            is_leaf = cl < 0
            v = np.zeros((tr.node_count, C), dtype=np.float64)
            v[:, :classes.size] = tr.value[:, 0, :]
            feat.append(np.where(is_leaf, -1, tr.feature))
            thr.append(np.where(is_leaf, 0.0, tr.threshold))
            lft.append(np.where(is_leaf, -1, cl + base))
            rgt.append(np.where(is_leaf, -1, cr + base))
            val.append(v)
            base += tr.node_count
        return cls.from_nodes(np.concatenate(feat), np.concatenate(thr), np.concatenate(lft), np.concatenate(rgt),
                              np.concatenate(val), np.array(roots), n_classes=C, classes_=classes)

    @classmethod
    def synthetic(cls, n_trees: int, depth: int, n_features: int, n_classes: int, seed: int = 1,
                  dist: str = "uniform", one_hot=None) -> "ProbabilityForest":
        """T complete depth-``depth`` trees for tests and benchmarks, tree by
        tree: the inner nodes as Forest.synthetic draws them (feature ~
        U{0..n_features-1}, threshold ~ U(0,1), or N(0,1) with dist="normal",
        as fp32), then the tree's leaf distributions ~ Dirichlet(1, ..., 1) (C
        unit exponentials, normalised by the quantisation); one table row per
        leaf, leaf (t, l) at row t 2^depth + l.  one_hot: (tree, leaf, class) triples whose
        leaves get the word 2^31 for that class and zero elsewhere (applied
        after every draw, so the other draws do not move)."""
        n_classes = int(n_classes)
        _check_soft_limits(int(n_trees), n_classes, int(depth))
        rng = np.random.default_rng(seed)
        n_inner, n_leaf = (1 << depth) - 1, 1 << depth
        inner = np.zeros((n_trees, n_inner, 2), dtype=np.int32)
        value = np.zeros((n_trees, n_leaf, n_classes), dtype=np.float64)
        for t in range(n_trees):
            f = rng.integers(0, n_features, size=n_inner)
            if dist == "uniform":
                th = rng.random(n_inner).astype(np.float32)
            else:
                th = rng.standard_normal(n_inner).astype(np.float32)
            inner[t, :, 0] = f
            inner[t, :, 1] = th.view(np.int32)
            value[t] = rng.standard_exponential((n_leaf, n_classes))
        for t, l, c in (one_hot or ()):
            value[t, l] = 0.0
            value[t, l, c] = 1.0
        leaf_id = np.arange(n_trees * n_leaf, dtype=np.int32).reshape(n_trees, n_leaf)
        return cls(inner=inner, leaf_id=leaf_id, leaf_q=quantize_distribution(value.reshape(-1, n_classes)),
                   depth=int(depth), n_classes=n_classes)


def _check_soft_limits(n_trees: int, n_classes: int, depth: int):
    if not 1 <= n_trees <= DAL_SOFT_MAX_TREES:
        raise ValueError(f"a soft-vote forest holds 1 to {DAL_SOFT_MAX_TREES} trees, not {n_trees}")
    if not 2 <= n_classes <= DAL_SOFT_MAX_CLASSES:
        raise ValueError(f"n_classes must lie in [2, {DAL_SOFT_MAX_CLASSES}], not {n_classes}")
    if not 1 <= depth <= DAL_SOFT_MAX_DEPTH:
        raise ValueError(f"tree depth must lie in [1, DAL_SOFT_MAX_DEPTH={DAL_SOFT_MAX_DEPTH}], not {depth}")
