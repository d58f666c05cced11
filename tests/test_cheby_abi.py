"""The Chebyshev step's entry points and the host side of the smoother (no GPU): the
symbols and the ABI version, the three-term recurrence against the Chebyshev
polynomials it is meant to produce, and the arguments it refuses."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb


def test_symbols_and_version():
    from poms_amd import _lib
    assert _lib.lib.poms_abi_version() >= 9
    names = _lib.header_symbols()
    for name in ("poms_op_cheby_step", "poms_op_cheby_supported"):
        assert name in names
        assert name in _lib._SIGS
        assert getattr(_lib.lib, name) is not None
    assert len(_lib._SIGS["poms_op_cheby_step"]) == 9


@pytest.mark.parametrize("degree", [1, 2, 7])
def test_polynomial_identity(degree):
    """On the scalar operator lam (D = 1) with b = 0 and x_0 = 1 the recurrence gives
    x_k = T_k((theta - lam)/delta) / T_k(sigma), inside the interval and outside it."""
    from poms_amd.solvers import chebyshev_coefficients
    lmin, lmax = 0.11, 3.3
    alpha, beta = chebyshev_coefficients(lmin, lmax, degree)
    assert len(alpha) == len(beta) == degree and beta[0] == 0.0
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    Tk = lambda t: npcheb.chebval(t, [0.0] * degree + [1.0])
    for lam in (lmin, 0.5, theta, 2.9, lmax, 0.5 * lmin, 0.01, 1.05 * lmax):
        xm, x = 0.0, 1.0
        for k in range(degree):
            xm, x = x, x + beta[k] * (x - xm) + alpha[k] * (0.0 - lam * x)
        want = Tk((theta - lam) / delta) / Tk(sigma)
        assert abs(x - want) <= 1e-13, (degree, lam, x, want)
        if lmin <= lam <= lmax:   # the min-max property: |x_k| <= 1 / T_k(sigma) on the interval
            assert abs(x) <= (1 + 1e-12) / Tk(sigma)


def test_refusals():
    from poms_amd.solvers import chebyshev_coefficients
    with pytest.raises(ValueError, match="lmin"):
        chebyshev_coefficients(0.0, 1.0, 3)
    with pytest.raises(ValueError, match="lmin"):
        chebyshev_coefficients(2.0, 2.0, 3)
    with pytest.raises(ValueError, match="degree"):
        chebyshev_coefficients(0.1, 3.0, 0)
