"""poms_amd.geometry without a device: the pull-back of a Jacobian (closed-form adjugate,
elementwise torch operations) against NumPy's linalg, the refusal of a non-positive
determinant, and the sampling order of a `Mapping`."""
import numpy as np
import pytest
import torch

from poms_amd.geometry import Mapping, pullback

PAIRS = {2: [(0, 0), (0, 1), (1, 1)], 3: [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]}


def random_jacobians(d, shape, seed):
    """identity + 0.2 uniform(0, 1): det >= 1 - O(0.2 d), well conditioned."""
    rng = np.random.default_rng(seed)
    return np.eye(d).reshape((d, d) + (1,) * len(shape)) + 0.2 * rng.uniform(0, 1, (d, d) + shape)


@pytest.mark.parametrize("d,shape", [(2, (7, 5)), (3, (4, 3, 5))])
def test_pullback_against_numpy_linalg(d, shape):
    """G = a det inv(J) inv(J)^T, gamma = c det, to 1e-14 relative (of the largest entry
    of G at the point; the matrices are well conditioned)."""
    J = random_jacobians(d, shape, 3 + d)
    rng = np.random.default_rng(1)
    a, c = rng.uniform(1, 2, shape), rng.uniform(0.5, 1.5, shape)
    Jt = [[torch.from_numpy(np.ascontiguousarray(J[i, k])) for k in range(d)] for i in range(d)]
    G, gamma, det = pullback(Jt, torch.from_numpy(a), torch.from_numpy(c))
    assert G.dtype == torch.float64 and tuple(G.shape) == (d * (d + 1) // 2,) + shape and G.is_contiguous()
    assert tuple(gamma.shape) == shape and tuple(det.shape) == shape
    Jm = np.moveaxis(J.reshape(d, d, -1), -1, 0)              # (points, d, d)
    dets = np.linalg.det(Jm)
    inv = np.linalg.inv(Jm)
    ref = a.reshape(-1, 1, 1) * dets.reshape(-1, 1, 1) * (inv @ np.swapaxes(inv, 1, 2))
    scale = np.abs(ref).max(axis=(1, 2))
    worst = 0.0
    for k, (i, j) in enumerate(PAIRS[d]):
        worst = max(worst, float(np.max(np.abs(G[k].numpy().reshape(-1) - ref[:, i, j]) / scale)))
    print(f"{d}D: worst relative error of G {worst:.2e}")
    assert worst <= 1e-14
    assert np.max(np.abs(det.numpy().reshape(-1) - dets) / dets) <= 1e-14
    assert np.max(np.abs(gamma.numpy().reshape(-1) - c.reshape(-1) * dets) / (c.reshape(-1) * dets)) <= 1e-14
    # one stacked tensor (d, d) + grid is taken as well; a = c = None: 1 and mass_coef
    G1, gamma1, _ = pullback(torch.from_numpy(J), mass_coef=0.5)
    assert float((G1 * torch.from_numpy(a) - G).abs().max()) <= 1e-14 * float(G.abs().max())
    assert torch.equal(gamma1, 0.5 * det)


def test_identity_jacobian_gives_the_identity_tensor():
    one, zero = torch.ones(3, 4, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64)
    G, gamma, det = pullback([[one, zero], [zero, one]])
    assert torch.equal(G[0], one) and torch.equal(G[1], zero) and torch.equal(G[2], one)
    assert torch.equal(det, one) and torch.equal(gamma, one)


@pytest.mark.parametrize("d", [2, 3])
def test_non_positive_determinant_raises(d):
    J = random_jacobians(d, (3,) * d, 5)
    J[(0, slice(None)) + (1,) * d] *= -1.0      # one point reflected
    with pytest.raises(ValueError, match="det"):
        pullback(torch.from_numpy(J))
    J = random_jacobians(d, (3,) * d, 5)
    J[(slice(None), slice(None)) + (0,) * d] = 0.0        # one point singular
    with pytest.raises(ValueError, match="det"):
        pullback(torch.from_numpy(J))
    with pytest.raises(ValueError, match="2 x 2 or 3 x 3"):
        pullback([[torch.ones(2, dtype=torch.float64)]])


def test_mapping_sampling_follows_indexing_ij():
    """F and jac see meshgrid(..., indexing='ij'): entry [i, j] belongs to point
    (points[0][i], points[1][j]).  The map x = xi0 + xi1^2 / 2, y = 2 xi1 has J = [[1,
    xi1], [0, 2]], det 2, adj = [[2, -xi1], [0, 1]], G = adj adj^T / 2."""
    F = lambda s, t: (s + 0.5 * t * t, 2.0 * t)
    jac = lambda s, t: [[1.0, t], [0.0, 2.0]]
    m = Mapping(F, jac)
    p0, p1 = np.array([0.1, 0.4, 0.8]), np.array([0.2, 0.3, 0.5, 0.9])
    x = m.physical([p0, p1], device="cpu")
    assert tuple(x[0].shape) == (3, 4)
    assert np.allclose(x[0].numpy(), p0[:, None] + 0.5 * p1[None, :] ** 2, rtol=0, atol=1e-16)
    assert np.array_equal(x[1].numpy(), np.broadcast_to(2.0 * p1[None, :], (3, 4)))
    # a: a function of the physical coordinates
    G, gamma, det = m.pullback([p0, p1], a=lambda x, y: 1.0 + x, c=lambda x, y: y, device="cpu")
    assert tuple(G.shape) == (3, 3, 4) and G.device.type == "cpu"
    a = 1.0 + p0[:, None] + 0.5 * p1[None, :] ** 2
    t = np.broadcast_to(p1[None, :], (3, 4))
    assert np.array_equal(det.numpy(), np.full((3, 4), 2.0))
    assert np.allclose(G[0].numpy(), a * (4.0 + t * t) / 2.0, rtol=1e-15, atol=0)
    assert np.allclose(G[1].numpy(), a * (-t) / 2.0, rtol=1e-15, atol=0)
    assert np.allclose(G[2].numpy(), a / 2.0, rtol=1e-15, atol=0)
    assert np.allclose(gamma.numpy(), 2.0 * 2.0 * t, rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="det"):
        Mapping(F, lambda s, t: [[1.0, t], [0.0, -2.0]]).pullback([p0, p1], device="cpu")
    with pytest.raises(TypeError):
        Mapping(F, None)
