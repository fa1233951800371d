"""The LAL dataset classes and their StandardScaler on the GPU.

Reference: lal_direct_mllib_implementation/classes/dataset.py.  Every
``Dataset*`` class there passes each split through MLlib's
``StandardScaler(withMean=True, withStd=True)`` (:163-173, :199-208, :228-236,
:257-271) and ``Dataset.setStartState`` (:56-130) seeds the labeled set with
one positive row, one negative row and a random fill.

The scaler here is exact (include/dal.h, "StandardScaler"): the
column sums of x and x*x are integers in limbs, added with 64-bit integer
atomics (csrc/scaler.hip), and mean and variance are each ONE rounding of an
exact rational, done on the host in Python integers.  The bits of mean, std
and of every standardised value are therefore the same for any row order, any
chunking and any shard count (dal.parallel.fit_scaler).

``std`` is the unbiased sample deviation (divisor n - 1), as in MLlib -- not
scikit-learn's ``StandardScaler`` (ddof = 0).
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from . import _lib
from ._lib import DAL_FLAG_NONFINITE, DAL_X_F32, DAL_X_F64, DalError

LIMB_BITS = 31
NO_LOW = np.iinfo(np.int32).max
NO_TOP = np.iinfo(np.int32).min
MAX_ROWS = (1 << 31) - 1


# ------------------------------------------------------------ host pieces --
def scaler_limbs(low, top):
    """(k1, k2, q int32 [d]) of a pool from its columns' (low, top) (the rule
    of csrc/scaler_exact.hpp, through dal_scaler_limbs), or DalError naming the
    first column whose squares span more than the exact sums hold."""
    low = np.ascontiguousarray(low, dtype=np.int32)
    top = np.ascontiguousarray(top, dtype=np.int32)
    d = int(low.shape[0])
    q = np.zeros(d, dtype=np.int32)
    k1, k2, bad = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(-1)
    rc = _lib.load().dal_scaler_limbs(low.ctypes.data, top.ctypes.data, d, ctypes.addressof(k1),
                                      ctypes.addressof(k2), q.ctypes.data, ctypes.addressof(bad))
    if rc != _lib.DAL_OK and bad.value >= 0:
        c = bad.value
        msg = _lib.load().dal_status_string(rc).decode()
        raise DalError(f"dal_scaler_limbs failed: {msg} (status {rc}): column {c} spans "
                       f"{int(top[c]) - int(low[c])} bits between its lowest and highest set bit, more than the "
                       f"{LIMB_BITS * _lib.DAL_RF_REG_MAX_LIMBS // 2} whose squares the exact sums hold")
    _lib.check(rc, "dal_scaler_limbs")
    return k1.value, k2.value, q


def _word_value(words) -> int:
    return sum(w << (LIMB_BITS * j) for j, w in enumerate(words))


def _rounded(num: int, den: int, e: int) -> float:
    """RN(num / den * 2^e): int / int true division is correctly rounded."""
    return (num << e) / den if e >= 0 else num / (den << -e)


def moments_from_cells(cells, q, k1: int, k2: int, n: int):
    """(mean, std) fp64 [d] from the exact cells int64 [d, k1 + k2] of n rows:
    mean = RN(S1 / n), var = RN((n S2 - S1^2) / (n (n - 1))) (0.0 for n == 1),
    std = sqrt(var).  Python integers, one correctly rounded division each."""
    rows = np.asarray(cells, dtype=np.int64).reshape(-1, k1 + k2).tolist()
    if n < 1:
        raise ValueError("a scaler needs at least one row")
    d = len(rows)
    mean, std = np.zeros(d, dtype=np.float64), np.zeros(d, dtype=np.float64)
    for c, (words, e) in enumerate(zip(rows, np.asarray(q).tolist())):
        s1, s2 = _word_value(words[:k1]), _word_value(words[k1:])
        mean[c] = _rounded(s1, n, e)
        if n >= 2:
            num = n * s2 - s1 * s1
            if num < 0:
                raise DalError(f"column {c}: the exact variance numerator is negative (corrupt cells)")
            std[c] = math.sqrt(_rounded(num, n * (n - 1), 2 * e))
    return mean, std


def scale_factor(std):
    """1.0 / std, 0.0 where std == 0.0 (the transform writes +0.0 there)."""
    std = np.asarray(std, dtype=np.float64)
    out = np.zeros_like(std)
    nz = std != 0.0
    out[nz] = 1.0 / std[nz]
    return out


def start_state(labels, n_start: int = 2, seed: int = 0):
    """Dataset.setStartState (dataset.py:56-130) with a fixed definition:
    positives and negatives by ascending index; rng = default_rng(seed);
    pos = rng.permutation(positives), neg = rng.permutation(negatives);
    known = [pos[0], neg[0]]; rest = rng.permutation(concat(pos[1:], neg[1:]));
    known += rest[:n_start - 2]; unknown = rest[n_start - 2:].  Returns
    (indices_known, indices_unknown) int64."""
    y = np.asarray(labels).reshape(-1)
    if n_start < 2:
        raise ValueError("n_start must be at least 2 (one row of each class)")
    if n_start > y.shape[0]:
        raise ValueError(f"n_start={n_start} exceeds the {y.shape[0]} rows")
    positives = np.flatnonzero(y == 1).astype(np.int64)
    negatives = np.flatnonzero(y == 0).astype(np.int64)
    if positives.size == 0 or negatives.size == 0:
        raise ValueError("the start state needs a row of each class (labels 1 and 0)")
    rng = np.random.default_rng(seed)
    pos, neg = rng.permutation(positives), rng.permutation(negatives)
    rest = rng.permutation(np.concatenate([pos[1:], neg[1:]]))
    known = np.concatenate([[pos[0], neg[0]], rest[:n_start - 2]]).astype(np.int64)
    return known, rest[n_start - 2:].astype(np.int64)


# ---------------------------------------------------------- device pieces --
def _device_rows(X, device=None):
    """X (numpy or torch, fp32, 2-D) as (device tensor, n, d, ldx): a device
    tensor whose rows are contiguous keeps its own leading dimension."""
    import torch

    from .engine import _require_cuda

    if isinstance(X, torch.Tensor):
        dev = _require_cuda(device if device is not None else (X.device if X.is_cuda else None))
        x = X
    else:
        dev = _require_cuda(device)
        x = torch.from_numpy(np.ascontiguousarray(X))
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("X must be a 2-D [rows, features] array with at least one feature")
    if x.dtype != torch.float32:
        raise ValueError("X must be fp32 (x*x of an fp64 value is not exact in fp64)")
    x = x.to(dev)
    n, d = int(x.shape[0]), int(x.shape[1])
    if n <= 1 or not (x.stride(1) == 1 and x.stride(0) >= d):
        x = x.contiguous()
    ldx = int(x.stride(0)) if n > 1 else d
    if n > MAX_ROWS:
        raise ValueError(f"{n} rows: the exact sums take at most {MAX_ROWS}")
    return x, n, d, ldx


def _chunks(n: int, chunk_rows):
    step = n if not chunk_rows else max(1, int(chunk_rows))
    a = 0
    while a < n:
        yield a, min(n, a + step)
        a += step


def _format_buffer(x, n: int, d: int, ldx: int, chunk_rows=None):
    """The format pass into one int32 device buffer [low (d), top (d), status (1)]."""
    import torch

    from .engine import _ptr, _stream

    buf = torch.empty(2 * d + 1, dtype=torch.int32, device=x.device)
    buf[:d].fill_(int(NO_LOW))
    buf[d:2 * d].fill_(int(NO_TOP))
    buf[2 * d:].zero_()
    base = _ptr(buf)
    for a, b in _chunks(n, chunk_rows):
        _lib.call("dal_scaler_format", _ptr(x) + 4 * a * ldx, b - a, d, ldx, base, base + 4 * d, base + 8 * d,
                  _stream(x.device))
    return buf


def device_format(x, n: int, d: int, ldx: int, chunk_rows=None):
    """The format pass over a device pool: (low, top) int32 [d] device tensors
    and the device status word (DAL_FLAG_NONFINITE)."""
    buf = _format_buffer(x, n, d, ldx, chunk_rows)
    return buf[:d], buf[d:2 * d], buf[2 * d:]


def device_accumulate(x, n: int, d: int, ldx: int, q, k1: int, k2: int, cells=None, chunk_rows=None):
    """cells int64 [d, k1 + k2] (device; zeros when not given) += the limbs
    of the pool's x and x*x.  q: int32 [d], host or device."""
    import torch

    from .engine import _ptr, _stream

    q_dev = torch.as_tensor(np.ascontiguousarray(q, dtype=np.int32)).to(x.device) \
        if not isinstance(q, torch.Tensor) else q.to(device=x.device, dtype=torch.int32).contiguous()
    if cells is None:
        cells = torch.zeros((d, k1 + k2), dtype=torch.int64, device=x.device)
    elif tuple(cells.shape) != (d, k1 + k2) or cells.dtype != torch.int64 or not cells.is_contiguous():
        raise ValueError(f"cells must be a contiguous int64 [{d}, {k1 + k2}] tensor")
    for a, b in _chunks(n, chunk_rows):
        _lib.call("dal_scaler_accumulate", _ptr(x) + 4 * a * ldx, b - a, d, ldx, _ptr(q_dev), k1, k2, _ptr(cells),
                  _stream(x.device))
    return cells


def check_format(low, top, status):
    """Host arrays of a finished format pass -> (k1, k2, q), ValueError for a
    non-finite value, DalError for a column over the span boundary."""
    if int(status) & DAL_FLAG_NONFINITE:
        raise ValueError("X must be finite: it holds a NaN or an infinity")
    return scaler_limbs(low, top)


class StandardScalerModel:
    """mean, std fp64 [d] (numpy) and the row count n of a fitted scaler."""

    def __init__(self, mean, std, n: int, with_mean: bool = True, with_std: bool = True):
        self.mean = np.ascontiguousarray(mean, dtype=np.float64)
        self.std = np.ascontiguousarray(std, dtype=np.float64)
        self.n = int(n)
        self.with_mean, self.with_std = bool(with_mean), bool(with_std)
        self._dev = {}

    def _operands(self, device):
        import torch

        ops = self._dev.get(device)
        if ops is None:
            ops = self._dev[device] = (torch.from_numpy(self.mean).to(device),
                                       torch.from_numpy(scale_factor(self.std)).to(device))
        return ops

    def transform(self, X, dtype=np.float32, device=None):
        """z = (double(x) - mean) * (1.0 / std), +0.0 where std == 0.0 (MLlib
        2.1's dense withMean && withStd branch; fp64, two roundings, no FMA),
        rounded to fp32 (the default) or kept as fp64.  Returns a device
        tensor [n, d] that PoolState and the select functions take directly."""
        import torch

        from .engine import _ptr, _stream

        f64 = dtype in (np.float64, torch.float64, "float64")
        if not f64 and dtype not in (np.float32, torch.float32, "float32"):
            raise ValueError("dtype must be float32 or float64")
        x, n, d, ldx = _device_rows(X, device)
        if d != self.mean.shape[0]:
            raise ValueError(f"X has {d} features, the scaler was fitted on {self.mean.shape[0]}")
        mean, factor = self._operands(x.device)
        out = torch.empty((n, d), dtype=torch.float64 if f64 else torch.float32, device=x.device)
        _lib.call("dal_scaler_transform", _ptr(x), n, d, ldx, _ptr(mean) if self.with_mean else None,
                  _ptr(factor) if self.with_std else None, _ptr(out), DAL_X_F64 if f64 else DAL_X_F32, d,
                  _stream(x.device))
        return out


class StandardScaler:
    """MLlib's StandardScaler(withMean, withStd) with exact column moments."""

    def __init__(self, with_mean: bool = True, with_std: bool = True):
        self.with_mean, self.with_std = bool(with_mean), bool(with_std)

    def fit(self, X, device=None, chunk_rows=None) -> StandardScalerModel:
        """X: numpy or torch fp32 [n, d], n >= 1.  ``chunk_rows`` feeds the
        kernels that many rows per call (the result does not depend on it).
        ValueError for a NaN or an infinity; DalError (DAL_ERR_UNSUPPORTED)
        naming the column when a column's values span more than 124 bits
        between their lowest and highest set bit."""
        x, n, d, ldx = _device_rows(X, device)
        if n < 1:
            raise ValueError("a scaler needs at least one row")
        fmt = _format_buffer(x, n, d, ldx, chunk_rows).cpu().numpy()  # one copy back: low, top, status
        k1, k2, q = check_format(fmt[:d], fmt[d:2 * d], fmt[2 * d])
        cells = device_accumulate(x, n, d, ldx, q, k1, k2, chunk_rows=chunk_rows)
        mean, std = moments_from_cells(cells.cpu().numpy(), q, k1, k2, n)
        return StandardScalerModel(mean, std, n, self.with_mean, self.with_std)


# ------------------------------------------------------------ the classes --
class Dataset:
    """A train and a test split with 0/1 labels (dataset.py:48-54).  After
    ``standardize`` the splits are device fp32 tensors."""

    def __init__(self, train_X, train_y, test_X=None, test_y=None):
        self.train_X, self.train_y = train_X, np.asarray(train_y)
        self.test_X, self.test_y = test_X, None if test_y is None else np.asarray(test_y)
        self.train_scaler = self.test_scaler = None
        self.n_start = None
        self.indices_known = self.indices_unknown = None

    @classmethod
    def from_text(cls, train_path, test_path=None, standardize: bool = True, test_scaler: str = "own",
                  device=None):
        """Read the reference's text files (features, then a 0/1 label) through
        dal.ingest with label_map="as_is" and, by default, standardise them."""
        from .ingest import parse_labeled_text

        Xtr, ytr = parse_labeled_text(train_path, label_map="as_is")
        Xte = yte = None
        if test_path is not None:
            Xte, yte = parse_labeled_text(test_path, label_map="as_is")
        ds = cls(Xtr, ytr, Xte, yte)
        if standardize:
            ds.standardize(test_scaler=test_scaler, device=device)
        return ds

    def standardize(self, test_scaler: str = "own", device=None):
        """Fit a StandardScaler on the train split and transform it; the test
        split is transformed by a scaler fitted on ITSELF for "own" (the
        reference: dataset.py:171) or by the train split's for "train"."""
        if test_scaler not in ("own", "train"):
            raise ValueError("test_scaler must be 'own' or 'train'")
        self.train_scaler = StandardScaler().fit(self.train_X, device=device)
        train = self.train_scaler.transform(self.train_X, device=device)
        if self.test_X is not None:
            self.test_scaler = self.train_scaler if test_scaler == "train" else \
                StandardScaler().fit(self.test_X, device=device)
            self.test_X = self.test_scaler.transform(self.test_X, device=device)
        self.train_X = train
        return self

    def set_start_state(self, n_start: int = 2, seed: int = 0):
        """See start_state.  Stores and returns (indices_known, indices_unknown)."""
        self.indices_known, self.indices_unknown = start_state(self.train_y, n_start, seed)
        self.n_start = int(n_start)
        return self.indices_known, self.indices_unknown


class _NamedDataset(Dataset):
    STEM = None

    def __init__(self, directory, standardize: bool = True, test_scaler: str = "own", device=None):
        from .ingest import parse_labeled_text

        Xtr, ytr = parse_labeled_text(os.path.join(directory, self.STEM + "_train.txt"), label_map="as_is")
        Xte, yte = parse_labeled_text(os.path.join(directory, self.STEM + "_test.txt"), label_map="as_is")
        Dataset.__init__(self, Xtr, ytr, Xte, yte)
        if standardize:
            self.standardize(test_scaler=test_scaler, device=device)


class DatasetCheckerboard2x2(_NamedDataset):
    """checkerboard2x2_{train,test}.txt (dataset.py:149-173)."""
    STEM = "checkerboard2x2"


class DatasetCheckerboard4x4(_NamedDataset):
    """checkerboard4x4_{train,test}.txt (dataset.py:188-210)."""
    STEM = "checkerboard4x4"


class DatasetRotatedCheckerboard2x2(_NamedDataset):
    """rotated_checkerboard2x2_{train,test}.txt (dataset.py:217-238)."""
    STEM = "rotated_checkerboard2x2"
