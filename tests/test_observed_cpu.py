"""Posterior on a subset of nodes with per-node noise (operator form 3), host side (no GPU): the algebra of
manifold_gp_amd/sampling.py in float64 against the dense Matern precision of the oracle, the exact GP on the observed subset,
the reduction to today's form-2 sampler, the C-ABI binding and the argument checks."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import _observed_ref as ref
from oracle.precision import dense_labeled_precision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]


def _fixture(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))


def _setup(case, norm, nu, frac=0.5, per_node=True, seed=0):
    g = _fixture(case)
    lo = ref.oracle(g, norm)
    Q2, R = ref.precision_root(lo, nu, float(g["kappa"]), 0.8, norm)
    rng = np.random.default_rng(seed)
    n = lo.n
    obs = rng.random(n) < frac
    s = 1e-2
    var = s * rng.uniform(0.5, 2.0, n) if per_node else np.full(n, s)
    return g, Q2, R, obs, var


@pytest.mark.parametrize("case", FIXTURES)
@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_perturbed_system_moments(case, norm, nu):
    """Cov(W y + s z + sqrt(s) W^1/2 w2) = s^2 R R^T + s W = s A3, so x = A3^-1 rhs has mean A3^-1 W y and covariance
    s A3^-1 = (Q2 + W / s)^-1 = P^-1 (the posterior precision's inverse)."""
    g, Q2, R, obs, var = _setup(case, norm, nu)
    s, w = ref.weights(var, obs)
    A3 = ref.system(Q2, w, s)
    cov_rhs = s * s * (R @ R.T) + s * np.diag(w)
    err = np.abs(cov_rhs - s * A3).max() / np.abs(s * A3).max()
    assert err < 1e-12, err
    A3inv = np.linalg.inv(A3)
    cov_x = A3inv @ cov_rhs @ A3inv
    Pinv = np.linalg.inv(Q2 + np.diag(w) / s)
    err = np.abs(cov_x - Pinv).max() / np.abs(Pinv).max()
    assert err < 1e-8, err
    # the mean: the rhs has expectation W y (z and w2 are zero-mean); NaN targets at unobserved nodes are never read
    y = g["train_y"].astype(np.float64)
    y_nan = np.where(obs, y, np.nan)
    m = ref.mean(Q2, y_nan, var, obs)
    assert np.isfinite(m).all()
    assert np.allclose(m, Pinv @ (np.where(obs, y, 0.0) / var * obs), rtol=1e-8, atol=1e-12 * np.abs(y).max())


@pytest.mark.parametrize("case", FIXTURES)
@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("frac", [0.1, 0.5])
def test_mean_at_observed_nodes_is_exact_gp(case, norm, frac):
    """At the observed nodes the mean is K_oo (K_oo + Sigma_oo)^-1 y_o with K = Q2^-1, whose observed block is the inverse of
    the Schur complement of Q2 (oracle/precision.py::dense_labeled_precision); the unobserved nodes get K_uo (K_oo +
    Sigma_oo)^-1 y_o; the covariance is the GP's conditional covariance."""
    g, Q2, _, obs, var = _setup(case, norm, 2, frac=frac, seed=3)
    y = g["train_y"].astype(np.float64)
    m = ref.mean(Q2, y, var, obs)
    K = np.linalg.inv(Q2)
    Koo = np.linalg.inv(dense_labeled_precision(Q2, obs))
    assert np.allclose(Koo, K[np.ix_(obs, obs)], rtol=1e-7, atol=1e-9 * np.abs(Koo).max())
    alpha = np.linalg.solve(Koo + np.diag(var[obs]), y[obs])
    want = K[:, obs] @ alpha
    err = np.abs(m - want).max() / np.abs(want).max()
    assert err < 1e-7, err
    s, w = ref.weights(var, obs)
    cov = s * np.linalg.inv(ref.system(Q2, w, s))
    want_cov = K - K[:, obs] @ np.linalg.solve(Koo + np.diag(var[obs]), K[obs, :])
    err = np.abs(cov - want_cov).max() / np.abs(want_cov).max()
    assert err < 1e-6, err


@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_all_observed_scalar_noise_is_form_2(norm, nu):
    """Every node observed at one noise s: s_ref = s, W = I, A3 = I + s Q2 and the rhs is y + s z + sqrt(s) w2 -- today's
    sampler (sampling.posterior_samples with a float noise)."""
    g, Q2, R, _, _ = _setup("dumbbell_k10_loop", norm, nu)
    n = Q2.shape[0]
    s = 3e-2
    obs, var = np.ones(n, bool), np.full(n, s)
    s_ref, w = ref.weights(var, obs)
    assert s_ref == s and (w == 1.0).all()
    assert np.array_equal(ref.system(Q2, w, s_ref), np.eye(n) + s * Q2)
    rng = np.random.default_rng(5)
    z, w2 = R @ rng.standard_normal((R.shape[1], 3)), rng.standard_normal((n, 3))
    y = g["train_y"].astype(np.float64)
    rhs = ref.perturbed_rhs(y, var, obs, z, w2)
    assert np.allclose(rhs, y[:, None] + s * z + np.sqrt(s) * w2, rtol=1e-14, atol=1e-14)


def test_reference_noise_does_not_change_the_answer():
    """s_ref is a scale of the system only: (W + s Q2)^-1 W y with W = s / Sigma is the same for any common s."""
    g, Q2, _, obs, var = _setup("dumbbell_k50_noloop", "randomwalk", 2, seed=9)
    y = g["train_y"].astype(np.float64)
    m = ref.mean(Q2, y, var, obs)
    for c in (0.5, 7.0):
        s = c * var[obs].min()
        w = np.where(obs, s / var, 0.0)
        assert np.allclose(np.linalg.solve(np.diag(w) + s * Q2, w * np.where(obs, y, 0.0)), m, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ host-side checks
def test_operator_struct_binding_has_trailing_obs_w():
    from manifold_gp_amd import _lib
    names = [f[0] for f in _lib.OperatorT._fields_]
    assert names[-1] == "obs_w" and names[:-1] == ["L", "pre", "post", "nu", "kappa", "scale", "form", "noise"]
    # the field sits behind the old struct's last byte: a caller built without it passes a shorter struct that the library
    # reads only for form 3
    assert _lib.OperatorT.obs_w.offset == _lib.OperatorT.noise.offset + 4 + 4 * (_lib.OperatorT.noise.offset % 8 == 0)
    assert ctypes.sizeof(_lib.OperatorT) == _lib.OperatorT.obs_w.offset + 8


def test_form_3_without_weights_is_an_argument_error():
    """obs_w == NULL with form 3: MGP_ERR_ARG before any device work (check_op); forms 0-2 never read the field."""
    from manifold_gp_amd import _lib
    op = _lib.OperatorT()
    buf = (ctypes.c_int32 * 8)(0, 4, 4, 4, 4, 4, 4, 4)
    vals = (ctypes.c_float * 4)()
    op.L.n, op.L.rowptr, op.L.col, op.L.vals, op.L.diag = 1, ctypes.addressof(buf), ctypes.addressof(buf), \
        ctypes.addressof(vals), ctypes.addressof(vals)
    op.nu, op.kappa, op.scale, op.noise = 2, 1.0, 1.0, 0.1
    fn = _lib.lib().mgp_operator_workspace_bytes
    op.form = 2
    assert fn(ctypes.byref(op), 1) > 0
    op.form = 3
    assert fn(ctypes.byref(op), 1) == 0                      # check_op refuses: no weights
    assert _lib.lib().mgp_operator_jacobi(ctypes.byref(op), None, None) == -1
    op.form = 4
    assert fn(ctypes.byref(op), 1) == 0


def _fake_desc():
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=2, kappa=1.0)


@pytest.mark.parametrize("noise,observed", [
    (0.1, torch.zeros(3, dtype=torch.bool)),                  # no observed node
    (0.1, torch.ones(4, dtype=torch.bool)),                   # wrong length
    (0.1, torch.ones(3)),                                     # not a bool mask
    (torch.full((4,), 0.1), None),                            # wrong length
    (torch.tensor([0.1, 0.0, 0.1]), None),                    # non-positive
    (torch.tensor([0.1, -1.0, 0.1]), torch.tensor([True, False, True])),   # non-positive at an unobserved node
    (torch.tensor([0.1, float("inf"), 0.1]), None),           # non-finite
    (torch.tensor([0.1, float("nan"), 0.1]), None),
    (float("inf"), torch.tensor([True, False, True])),
    (0.0, torch.tensor([True, False, True])),
])
def test_observed_argument_checks(noise, observed):
    from manifold_gp_amd import sampling
    d = _fake_desc()
    for fn in (lambda: sampling.posterior_mean(d, torch.zeros(3), noise, observed=observed),
               lambda: sampling.posterior_samples(d, torch.zeros(3), noise, 2, 1, observed=observed),
               lambda: sampling.posterior_rhs(d, torch.zeros(3), noise, 2, 1, observed=observed)):
        with pytest.raises(ValueError):
            fn()


def test_observation_weights_follow_the_definition():
    from manifold_gp_amd import sampling
    d = _fake_desc()
    var = torch.tensor([0.4, 0.1, 0.2])
    obs = torch.tensor([True, False, True])
    ob = sampling._observation(d, var, obs)
    assert ob.s_ref == pytest.approx(0.2)
    assert torch.allclose(ob.w.view(-1), torch.tensor([0.5, 0.0, 1.0]))
    assert torch.allclose(ob.sigma.view(-1), var.sqrt())
    # today's path: one noise (a python float or a one-element tensor such as likelihood.noise) and every node observed,
    # with today's checks (positive; an infinite noise was and is accepted there)
    assert sampling._observation(d, 0.1, None) is None
    assert sampling._observation(d, 0.1, torch.ones(3, dtype=torch.bool)) is None
    assert sampling._observation(d, torch.tensor([0.1]), None) is None
    assert sampling._observation(d, torch.tensor(0.1), None) is None
    assert sampling._observation(d, float("inf"), None) is None
    ob = sampling._observation(d, torch.tensor([0.1]), obs)
    assert ob.s_ref == pytest.approx(0.1) and torch.equal(ob.w.view(-1), torch.tensor([1.0, 0.0, 1.0]))
    # a scalar noise with a mask, a noise vector without one: form 3
    ob = sampling._observation(d, 0.1, obs)
    assert ob.s_ref == pytest.approx(0.1) and torch.equal(ob.w.view(-1), torch.tensor([1.0, 0.0, 1.0]))
    ob = sampling._observation(d, var, None)
    assert torch.allclose(ob.w.view(-1), torch.tensor([0.25, 1.0, 0.5]))


def test_model_methods_take_observed():
    import inspect
    from manifold_gp_amd.models import RiemannGP
    for name in ("sample_posterior", "precision_posterior_mean"):
        assert "observed" in inspect.signature(getattr(RiemannGP, name)).parameters
