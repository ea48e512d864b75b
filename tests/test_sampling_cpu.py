"""Exact GMRF sampling, host side (no GPU): the generator's known answers, the sparse factor G G^T = tau I + L_sym, the
sampling algebra of manifold_gp_amd/sampling.py in float64 against the dense Matern precision of the oracle, and the
argument checks of the Python layer and the C-ABI binding."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from _sampling_ref import box_muller, edge_factor, philox4x32, seed_key
from oracle.laplacian import LaplacianOracle
from oracle.precision import dense_matern_precision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]


def _fixture(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def _oracle(g, norm):
    return LaplacianOracle(g["edge_value"], g["edge_index"], g["train_x"].shape[0], float(g["eps"]), norm,
                           bool(g["self_loops"]), dtype=np.float64)


def _factor(lo):
    """(dense L_sym, E) in float64 from the oracle's COO edges (each once, r < c)."""
    r, c = lo.idx[0], lo.idx[1]
    assert (r < c).all()
    return lo.dense_symmetric(), edge_factor(lo.n, r, c, lo.triu, np.sqrt(lo.degree))


# ------------------------------------------------------------------------------------------------ generator
@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    out = philox4x32(np.array(ctr, np.uint32), np.array(key, np.uint32))
    assert [int(v) for v in out] == want


def test_seed_key_and_box_muller_moments():
    assert list(seed_key(0x0123456789abcdef)) == [0x89abcdef, 0x01234567]
    rng = np.random.default_rng(0)
    words = rng.integers(0, 2 ** 32, size=(50000, 4), dtype=np.uint64).astype(np.uint32)
    z = np.stack([box_muller(words, np.full(len(words), s)) for s in range(4)], axis=1)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.02
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.02            # the two halves of one Box-Muller pair


# ------------------------------------------------------------------------------------------------ the factor
@pytest.mark.parametrize("case", FIXTURES)
def test_sparse_factor_reproduces_tau_plus_laplacian(case):
    g = _fixture(case)
    lo = _oracle(g, "symmetric")
    L, E = _factor(lo)
    tau = 2.0 * 3 / float(g["kappa"]) ** 2
    A = tau * np.eye(lo.n) + L
    Gm = np.hstack([np.sqrt(tau) * np.eye(lo.n), E])
    err = np.abs(Gm @ Gm.T - A).max() / np.abs(A).max()
    assert err <= 1e-13, err


# ------------------------------------------------------------------------------------------------ the algebra
def _pieces(lo, nu, kappa, scale, norm):
    L, E = _factor(lo)
    n = lo.n
    tau = 2.0 * nu / kappa ** 2
    A = tau * np.eye(n) + L
    Gm = np.hstack([np.sqrt(tau) * np.eye(n), E])
    P = np.sqrt(lo.degree) if norm == "randomwalk" else np.ones(n)
    Q2 = scale * dense_matern_precision(lo.dense(), nu, kappa, lo.degree if norm == "randomwalk" else None)
    return A, Gm, P, Q2


def _mpow(A, k):
    return np.linalg.matrix_power(A, k) if k > 0 else np.eye(A.shape[0])


@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("nu", [1, 2, 3, 4])
def test_precision_root_and_prior_covariance(norm, nu):
    """z = R w with R R^T = Q2 and f = F w with F F^T = Q2^-1 (the maps precision_samples / prior_samples apply)."""
    g = _fixture("dumbbell_k10_loop")
    lo = _oracle(g, norm)
    kappa, scale = float(g["kappa"]), 0.37
    A, Gm, P, Q2 = _pieces(lo, nu, kappa, scale, norm)
    if nu % 2:
        R = np.sqrt(scale) * P[:, None] * (_mpow(A, (nu - 1) // 2) @ Gm)
        F = (1.0 / np.sqrt(scale)) * (1.0 / P)[:, None] * np.linalg.solve(_mpow(A, (nu + 1) // 2), Gm)
    else:
        R = np.sqrt(scale) * P[:, None] * _mpow(A, nu // 2)
        F = (1.0 / np.sqrt(scale)) * (1.0 / P)[:, None] * np.linalg.inv(_mpow(A, nu // 2))
    err_r = np.abs(R @ R.T - Q2).max() / np.abs(Q2).max()
    assert err_r < 1e-12, err_r
    # Cov(f) Q2 = I
    err_f = np.abs((F @ F.T) @ Q2 - np.eye(lo.n)).max()
    assert err_f < 1e-8, err_f


@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("nu", [1, 2])
def test_posterior_perturbation_covariance(norm, nu):
    """eta = z + s^-1/2 w2 has covariance Q2 + I/s = Pp (the posterior precision), so x = (I + s Q2)^-1 (y + s eta) =
    Pp^-1 (y / s + eta) has covariance Pp^-1 Cov(eta) Pp^-1 = Pp^-1."""
    g = _fixture("dumbbell_k50_noloop")
    lo = _oracle(g, norm)
    s, scale = 0.05, 2.5
    A, Gm, P, Q2 = _pieces(lo, nu, float(g["kappa"]), scale, norm)
    R = np.sqrt(scale) * P[:, None] * (_mpow(A, (nu - 1) // 2) @ Gm if nu % 2 else _mpow(A, nu // 2))
    cov_eta = R @ R.T + np.eye(lo.n) / s
    Pp = Q2 + np.eye(lo.n) / s
    Pinv = np.linalg.inv(Pp)
    err = np.abs(Pinv @ cov_eta @ Pinv - Pinv).max() / np.abs(Pinv).max()
    assert err < 1e-10, err
    # the mean is the headline solve: (I + s Q2)^-1 y = Pp^-1 y / s
    y = g["train_y"].astype(np.float64)
    assert np.allclose(np.linalg.solve(np.eye(lo.n) + s * Q2, y), Pinv @ y / s, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ host-side checks
def test_gmrf_noise_binding_matches_header():
    from manifold_gp_amd import _lib
    res, args = _lib.SIGNATURES["mgp_gmrf_noise"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.CsrT), ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                    ctypes.c_uint64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    fn = _lib.lib().mgp_gmrf_noise
    assert fn.argtypes == args
    # argument errors are reported before anything touches a device
    csr = _lib.CsrT()
    assert fn(None, None, 1.0, 0, 0, 1, 0, 4, None, None) == -1
    assert fn(ctypes.byref(csr), None, 1.0, 0, 0, 1, 0, 4, None, None) == -1


def _fake_desc(**kw):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    base = dict(data=data, nu=2, kappa=1.0)
    base.update(kw)
    return Descriptor(**base), sq


def test_sampling_rejects_unsupported_descriptors():
    from manifold_gp_amd import sampling
    d, sq = _fake_desc(form=2, noise=0.1)
    for fn in (lambda: sampling.precision_samples(d, 4, 1), lambda: sampling.prior_samples(d, 4, 1),
               lambda: sampling.posterior_samples(d, torch.zeros(3), 0.1, 4, 1)):
        with pytest.raises(NotImplementedError):
            fn()
    masked, _ = _fake_desc(pre=torch.ones(3), post=torch.ones(3))         # a 0/1 mask folded into pre / post
    with pytest.raises(NotImplementedError):
        sampling.precision_samples(masked, 4, 1)
    with pytest.raises(NotImplementedError):
        sampling.precision_samples(None, 4, 1)
    half, _ = _fake_desc(pre=sq)
    with pytest.raises(NotImplementedError):
        sampling.prior_samples(half, 4, 1)
    with pytest.raises(NotImplementedError):
        sampling.precision_samples(_fake_desc(nu=0)[0], 4, 1)


@pytest.mark.parametrize("bad", [
    dict(S=0), dict(S=2.0), dict(S=True), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(offset=-4),
    dict(tag=1), dict(tag=4),
])
def test_gmrf_noise_argument_checks(bad):
    from manifold_gp_amd import sampling
    args = dict(data=None, S=4, seed=7, offset=0, tag=0)
    args.update(bad)
    with pytest.raises(ValueError):
        sampling.gmrf_noise(**args)


def test_sample_counts_and_noise_checked():
    from manifold_gp_amd import sampling
    d, _ = _fake_desc()
    with pytest.raises(ValueError):
        sampling.precision_samples(d, 0, 1)
    with pytest.raises(ValueError):
        sampling.prior_samples(d, -3, 1)
    with pytest.raises(ValueError):
        sampling.posterior_samples(d, torch.zeros(3), 0.0, 4, 1)
    with pytest.raises(ValueError):
        sampling.posterior_mean(d, torch.zeros(3), -1.0)


def test_seed_none_follows_torch_manual_seed():
    from manifold_gp_amd import sampling
    torch.manual_seed(123)
    a = sampling.draw_seed()
    torch.manual_seed(123)
    assert sampling.draw_seed() == a and 0 <= a < 2 ** 63


def test_public_sampling_methods_exist():
    from manifold_gp_amd.models import RiemannGP
    from manifold_gp_amd.operators import PrecisionMaternOperator, ScaleWrapperOperator
    for cls, names in ((PrecisionMaternOperator, ["zero_mean_mvn_samples"]),
                       (ScaleWrapperOperator, ["zero_mean_mvn_samples"]),
                       (RiemannGP, ["sample_prior", "sample_posterior", "precision_posterior_mean"])):
        for name in names:
            assert callable(getattr(cls, name, None)), "%s.%s" % (cls.__name__, name)
