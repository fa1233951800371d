"""The H.H symmetric Gram's algebra (csrc/gram_sym.hip), restated in NumPy on
exact integers (CPU only): over super-block pairs taken by the orientation
rule the MFMAs form the row sums of H_P H_Q^T alone; the closed form of
dal_gram_sym_residual -- <L_r, S~> + <H_r, S^L + CH_B>, with S^L the sum of L
and S~ the sum of u~ = H + L over every row and CH_B the parity-class prefix
sum of the sigma^H of the other super blocks taking B, as csym_scan_kernel
forms them from one int64 per (super block, feature) and two totals --
completes every row to sum_j <u~_r, u~_j> exactly.
tests/test_gram_compensation.py records the algebra before (H.H + H.L on the
MFMAs).  Reference: density_weighting.py:67-75,157-161."""
import numpy as np
import pytest

SB = 512


def takes(P, Q):
    return Q == P or (Q > P and (P + Q) % 2 == 0) or (Q < P and (P + Q) % 2 == 1)


def residual(H, L, nsb):
    D = H.shape[1]
    sig_h = np.array([H[q * SB:(q + 1) * SB].sum(0) for q in range(nsb)])  # the workspace's sig region
    s_l = L.sum(0)                                                          # accumulated beside it
    tot = [sig_h[0::2].sum(0), sig_h[1::2].sum(0)]
    s_t = tot[0] + tot[1] + s_l                                             # S~
    e = [np.zeros(D, dtype=np.int64) for _ in range(2)]
    res = np.zeros(H.shape[0], dtype=np.int64)
    for q in range(nsb):
        b = q & 1
        ch = e[b] + tot[1 - b] - e[1 - b]      # sigma^H over the other super blocks taking q
        rows = slice(q * SB, (q + 1) * SB)
        res[rows] = L[rows] @ s_t + H[rows] @ (s_l + ch)
        e[b] = e[b] + sig_h[q]
    return res


@pytest.mark.parametrize("nsb,D,seed", [(1, 4, 0), (2, 8, 1), (3, 5, 4), (7, 8, 2), (10, 3, 3)])
def test_hh_sym_gram_completes_every_row(nsb, D, seed):
    rng = np.random.default_rng(seed)
    n = nsb * SB
    H = rng.integers(-2048, 2048, (n, D)).astype(np.int64)
    L = rng.integers(-2, 3, (n, D)).astype(np.int64)
    zero = rng.random(n) < 0.05  # excluded / padding rows are zero rows
    H[zero] = 0
    L[zero] = 0
    U = H + L
    acc = np.zeros(n, dtype=np.int64)
    for P in range(nsb):
        for Q in range(nsb):
            if not takes(P, Q):
                continue
            T = H[P * SB:(P + 1) * SB] @ H[Q * SB:(Q + 1) * SB].T
            acc[P * SB:(P + 1) * SB] += T.sum(axis=1)  # row sums only (the kernel)
    full = U @ U.sum(axis=0)
    assert np.array_equal(acc + residual(H, L, nsb), full)
    if nsb > 1:
        assert not np.array_equal(acc, full)  # the remainder is not negligible in this test


def test_ch_is_the_sum_over_the_other_takers():
    """The prefix rule of CH_B against its definition."""
    rng = np.random.default_rng(5)
    for nsb in (1, 2, 3, 7, 10):
        sig = rng.integers(-1000, 1000, (nsb, 4)).astype(np.int64)
        tot = [sig[0::2].sum(0), sig[1::2].sum(0)]
        e = [np.zeros(4, dtype=np.int64) for _ in range(2)]
        for B in range(nsb):
            b = B & 1
            direct = sum((sig[P] for P in range(nsb) if P != B and takes(P, B)), np.zeros(4, dtype=np.int64))
            assert np.array_equal(e[b] + tot[1 - b] - e[1 - b], direct)
            e[b] = e[b] + sig[B]
