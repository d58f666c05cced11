"""The eigensolver without a GPU: the two block entry points at the C boundary, the small
dense Rayleigh-Ritz step against scipy, and lobpcg's refusals that come before any device
work."""
import re

import numpy as np
import pytest
import scipy.linalg as sla

from poms_amd import _lib
from poms_amd.eigen import GramNotPositiveDefinite, lobpcg, rayleigh_ritz

EPS = 2.0 ** -52


def test_block_entry_points_are_declared():
    syms = _lib.header_symbols()
    for name, nargs in (("poms_block_gram", 9), ("poms_block_combine", 8)):
        assert name in syms
        assert len(_lib._SIGS[name]) == nargs
        assert hasattr(_lib.lib, name)
    assert _lib.lib.poms_abi_version() >= 13
    text = _lib.HEADER_PATH.read_text()
    assert int(re.search(r"#define POMS_ABI_VERSION (\d+)", text).group(1)) >= 13
    assert int(re.search(r"#define POMS_BLOCK_MAX (\d+)", text).group(1)) == 24


def test_block_entry_points_refuse_null_arguments():
    assert _lib.lib.poms_block_gram(None, None, 1, None, 1, None, 0, None, None) != 0
    assert _lib.lib.poms_last_error() != b""
    with pytest.raises(_lib.PomsError):
        _lib.call("poms_block_combine", None, None, 1, None, 1, None, None, None)


def spd_pair(n, seed):
    """A seeded basis S (60 x n) with an SPD pair (A, B) of size 60: G = SᵀAS, H = SᵀBS."""
    rng = np.random.default_rng(seed)
    N = 60
    Q = rng.standard_normal((N, N))
    A = Q @ np.diag(rng.uniform(1.0, 50.0, N)) @ Q.T / N
    R = rng.standard_normal((N, N))
    B = R @ np.diag(rng.uniform(0.5, 2.0, N)) @ R.T / N
    S = rng.standard_normal((N, n))
    return S, A, B


@pytest.mark.parametrize("n", [4, 8, 12])
def test_rayleigh_ritz_against_scipy(n):
    S, A, B = spd_pair(n, 100 + n)
    G, H = S.T @ A @ S, S.T @ B @ S
    G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
    want = sla.eigh(G, H, eigvals_only=True)
    m = max(1, n // 3)
    theta, C, cond = rayleigh_ritz(G, H, m)
    assert theta.shape == (m,) and C.shape == (n, m)
    assert np.all(np.diff(theta) >= 0.0)
    assert np.max(np.abs(theta - want[:m])) <= n * EPS * want[-1]
    d = 1.0 / np.sqrt(np.diag(H))
    assert cond == pytest.approx(np.linalg.cond(d[:, None] * H * d[None, :]), rel=1e-10)
    # H-orthonormal coefficients, Ritz pairs of the pencil
    assert np.max(np.abs(C.T @ H @ C - np.eye(m))) <= 8 * n * EPS * cond
    assert np.max(np.abs(C.T @ G @ C - np.diag(theta))) <= 8 * n * EPS * cond * want[-1]


@pytest.mark.parametrize("n", [4, 8, 12])
def test_rayleigh_ritz_does_not_depend_on_the_basis_lengths(n):
    S, A, B = spd_pair(n, 200 + n)
    G, H = S.T @ A @ S, S.T @ B @ S
    want = sla.eigh(0.5 * (G + G.T), 0.5 * (H + H.T), eigvals_only=True)
    m = max(1, n // 3)
    base = rayleigh_ritz(G, H, m)[0]
    for i, e in ((0, 6), (n - 1, -6), (n // 2, 6)):
        s = np.ones(n)
        s[i] = 10.0 ** e
        S2 = S * s
        G2, H2 = S2.T @ A @ S2, S2.T @ B @ S2
        theta, C, cond = rayleigh_ritz(G2, H2, m)
        assert np.max(np.abs(theta - want[:m])) <= n * EPS * want[-1]
        assert np.max(np.abs(theta - base)) <= n * EPS * want[-1]
        assert np.max(np.abs(C.T @ H2 @ C - np.eye(m))) <= 8 * n * EPS * cond


def test_rayleigh_ritz_refuses_a_dependent_basis():
    S, A, B = spd_pair(8, 7)
    S[:, 5] = S[:, 2]
    with pytest.raises(GramNotPositiveDefinite):
        rayleigh_ritz(S.T @ A @ S, S.T @ B @ S, 3)
    assert issubclass(GramNotPositiveDefinite, np.linalg.LinAlgError)
    H = np.eye(4)
    H[2, 2] = 0.0
    with pytest.raises(GramNotPositiveDefinite):
        rayleigh_ritz(np.eye(4), H, 2)
    with pytest.raises(ValueError):
        rayleigh_ritz(np.eye(4), np.eye(4), 5)


@pytest.mark.parametrize("k", [0, 9, -1, 2.5])
def test_lobpcg_refuses_block_sizes_before_any_device_work(k):
    # (A is never looked at: k is checked first, so no device is needed)
    with pytest.raises(ValueError, match="k"):
        lobpcg(object(), k=k)
