"""Marginal posterior variances in precision form, host side (no GPU): the diagonal formulas of csrc/variance.hip against
the dense float64 Matern precision, the single-site Rao-Blackwell estimator of sampling.posterior_variance in float64 on
the Philox restatement of the sampler's noise against diag((Q2 + W / s)^-1), the C-ABI argument checks and the Python
argument checks.  Setting of the statistical tests (docs/kernels/sampling.md, "Marginal variances"): kappa = 0.5,
scale 1.3, per-node noise variances drawn from {1e-2, 4e-2}, every node or 10 % of the nodes observed, seed 0, S = 64."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import _observed_ref as oref
import _variance_ref as vref

FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]
NORMS = ["symmetric", "randomwalk"]
KAPPA, SCALE, SEED, S = 0.5, 1.3, 0, 64


# ------------------------------------------------------------------------------------------------ 1: the diagonal
@pytest.mark.parametrize("case", FIXTURES)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_diagonal_formulas_match_dense_precision(golden, case, norm, nu):
    """diag(A), diag(A^2), diag(A^3) by the neighbour and triangle sums against the diagonal of the dense float64 Q2
    (_observed_ref.precision_root), for operator forms 0, 2 and 3 (10 % observed, per-node noise): 1e-12 relative."""
    g = golden(case)
    lo = oref.oracle(g, norm)
    Q2, _ = oref.precision_root(lo, nu, KAPPA, SCALE, norm)
    q = vref.q2_diag(lo, nu, KAPPA, SCALE, norm)
    rng = np.random.default_rng(nu)
    obs = rng.random(lo.n) < 0.1
    s, w = oref.weights(rng.choice([1e-2, 4e-2], lo.n), obs)
    wants = {0: np.diag(Q2), 2: np.diag(np.eye(lo.n) + s * Q2), 3: np.diag(oref.system(Q2, w, s))}
    for form, want in wants.items():
        got = vref.system_diag(q, form, s, w)
        err = np.abs(got - want).max() / np.abs(want).max()
        rel = np.abs(got / want - 1.0).max()
        print("form %d: max error %.2e of the largest entry, %.2e entrywise" % (form, err, rel))
        assert rel <= 1e-12, (form, rel)


def test_triangle_term_on_a_hand_built_graph():
    """Five nodes: the triangle 0-1-2, the pendant edge 2-3 and the isolated node 4.  The triangle term of diag(A^3) is
    2 S_01 S_12 S_20 at the three corners and 0 elsewhere."""
    S_ = np.zeros((5, 5))
    for i, j, v in [(0, 1, 0.5), (1, 2, 0.25), (0, 2, 2.0), (2, 3, 1.5)]:
        S_[i, j] = S_[j, i] = v
    a = np.array([3.0, 4.0, 5.0, 6.0, 7.0])
    A = np.diag(a) - S_
    for nu in (1, 2, 3):
        assert np.allclose(vref.diag_power(a, S_, nu), np.diag(np.linalg.matrix_power(A, nu)), rtol=1e-14, atol=0)
    no_tri = a ** 3 + 2 * a * (S_ * S_).sum(1) + (S_ * S_) @ a
    assert np.allclose(no_tri - vref.diag_power(a, S_, 3), [0.5, 0.5, 0.5, 0.0, 0.0], rtol=1e-14, atol=1e-14)


# ------------------------------------------------------------------------------------------------ 2-5: the estimator
_DRAWS = {}       # Philox normals per fixture (they depend on the seed, S and the edge list alone)
_RESULTS = {}


def _case(golden, case, norm, nu, frac):
    """(truth, (var, se) Rao-Blackwell, (var, se) plain) of one case, computed once per session."""
    key = (case, norm, nu, frac)
    if key not in _RESULTS:
        g = golden(case)
        dense = vref.Dense(g, norm, nu, SCALE, KAPPA)
        n = dense.n
        var = np.random.default_rng(1).choice([1e-2, 4e-2], n)
        obs = np.ones(n, bool) if frac == 1.0 else np.random.default_rng(2).random(n) < frac
        s, w = oref.weights(var, obs)
        cache = _DRAWS.setdefault(case, {})
        _RESULTS[key] = (vref.truth(dense.Q2, w, s), vref.reference(dense, var, obs, SEED, S, "rao-blackwell", cache),
                         vref.reference(dense, var, obs, SEED, S, "samples", cache))
    return _RESULTS[key]


def _rms(v, truth):
    return float(np.sqrt(((v / truth - 1.0) ** 2).mean()))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("frac", [1.0, 0.1])
def test_rao_blackwell_reproduces_the_marginal_variance(golden, norm, nu, frac):
    """dumbbell_k50_noloop, seed 0, S = 64: within 2e-2 relative of diag(P^-1) at every node (5 x the 3.6e-3 measured with
    numpy draws; the Philox draws give at most 2.5e-3), and at most 1 % of the nodes outside 4 se of the truth."""
    truth, (v, se), _ = _case(golden, "dumbbell_k50_noloop", norm, nu, frac)
    rel = np.abs(v / truth - 1.0)
    outside = float((np.abs(v - truth) > 4.0 * se).mean())
    print("rms %.2e worst node %.2e; outside 4 se: %.4f of the nodes" % (_rms(v, truth), rel.max(), outside))
    assert rel.max() <= 2e-2, rel.max()
    assert outside <= 0.01, outside


@pytest.mark.parametrize("case", FIXTURES)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("frac", [1.0, 0.1])
def test_rao_blackwell_is_never_worse_than_plain_and_se_is_positive(golden, case, norm, nu, frac):
    truth, (v, se), (vp, sep) = _case(golden, case, norm, nu, frac)
    print("rao-blackwell rms %.2e worst %.2e | plain rms %.2e worst %.2e | median se / var %.2e | %.2e"
          % (_rms(v, truth), np.abs(v / truth - 1).max(), _rms(vp, truth), np.abs(vp / truth - 1).max(),
             np.median(se / v), np.median(sep / vp)))
    assert _rms(v, truth) <= _rms(vp, truth)
    assert (se > 0).all() and (sep > 0).all()
    assert (v > 0).all()


def test_estimator_identity_in_expectation(golden):
    """E[v] = diag(P^-1): e = (A3^-1 - D^-1) p with Cov p = s A3, so Cov e = s M A3 M, M = A3^-1 - D^-1, and
    s / d_i + (Cov e)_ii = s (A3^-1)_ii, evaluated with dense matrices."""
    g = golden("dumbbell_k10_loop")
    dense = vref.Dense(g, "randomwalk", 3, SCALE, KAPPA)
    n = dense.n
    rng = np.random.default_rng(4)
    obs = rng.random(n) < 0.1
    s, w = oref.weights(rng.choice([1e-2, 4e-2], n), obs)
    A3 = oref.system(dense.Q2, w, s)
    d = np.diag(A3)
    Ainv = np.linalg.inv(A3)
    M = Ainv - np.diag(1.0 / d)
    ee = s * ((M @ A3) * M).sum(1)                       # diag(s M A3 M), M symmetric
    assert np.allclose(s / d + ee, s * np.diag(Ainv), rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ host-side checks
def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    acc = (ctypes.c_double * 4)()
    u, a = ctypes.addressof(buf), ctypes.addressof(acc)
    for C in (0, -1, 257):
        assert lib.mgp_row_moments(u, None, None, None, 2, C, a, None) == -1
    assert lib.mgp_row_moments(None, None, None, None, 2, 4, a, None) == -1
    assert lib.mgp_row_moments(u, None, None, None, 2, 4, None, None) == -1
    assert lib.mgp_row_moments(u, None, None, u, 2, 4, a, None) == -1          # Pm without rdiag
    assert lib.mgp_row_moments(u, None, None, None, 0, 4, a, None) == -1
    op = _lib.OperatorT()
    idx = (ctypes.c_int32 * 8)(0, 4, 4, 4, 4, 4, 4, 4)
    op.L.n, op.L.rowptr, op.L.col, op.L.vals, op.L.diag = 1, ctypes.addressof(idx), ctypes.addressof(idx), u, u
    op.nu, op.kappa, op.scale, op.noise, op.form = 2, 1.0, 1.0, 0.1, 2
    fn = lib.mgp_operator_diag_exact
    assert lib.mgp_operator_diag_exact_workspace_bytes(ctypes.byref(op)) == 0
    assert fn(None, a, None, 0, None) == -1 and fn(ctypes.byref(op), None, None, 0, None) == -1
    op.nu = 4
    assert fn(ctypes.byref(op), a, None, 0, None) == -3
    op.nu, op.form = 3, 1
    assert fn(ctypes.byref(op), a, None, 0, None) == -3
    op.form = 3
    assert fn(ctypes.byref(op), a, None, 0, None) == -1                        # form 3 without weights
    op.form, op.L.n = 2, 2 ** 31
    assert fn(ctypes.byref(op), a, None, 0, None) == -1
    op.L.n, op.L.col = 1, None
    assert fn(ctypes.byref(op), a, None, 0, None) == -1


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_posterior_variance_argument_checks():
    from manifold_gp_amd import sampling
    d = _fake_desc()
    for fn in (sampling.posterior_variance, sampling.posterior_stddev):
        with pytest.raises(ValueError):
            fn(d, 0.1, method="control-variate")
        with pytest.raises(ValueError):
            fn(d, 0.1, S=0)
        with pytest.raises(ValueError):
            fn(d, 0.0)
        with pytest.raises(ValueError):
            fn(d, 0.1, observed=torch.zeros(3, dtype=torch.bool))
        with pytest.raises(ValueError):
            fn(d, torch.tensor([0.1, -1.0, 0.1]))
        with pytest.raises(NotImplementedError, match="samples"):
            fn(_fake_desc(nu=4), 0.1)
        with pytest.raises(NotImplementedError):
            fn(_fake_desc(form=1), 0.1)
        masked = d.masked(torch.tensor([1.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 1.0]))
        with pytest.raises(NotImplementedError):
            fn(masked, 0.1)
    sig = inspect.signature(sampling.posterior_variance)
    assert list(sig.parameters) == ["desc", "noise", "S", "seed", "observed", "method", "noisy", "tol", "refine", "max_iter"]
    assert (sig.parameters["S"].default, sig.parameters["method"].default, sig.parameters["tol"].default,
            sig.parameters["refine"].default, sig.parameters["max_iter"].default) == (64, "rao-blackwell", 1e-6, 1, 5000)


def test_model_methods_exist_with_the_documented_signature():
    from manifold_gp_amd.models import RiemannGP
    for name in ("precision_posterior_variance", "precision_posterior_stddev"):
        sig = inspect.signature(getattr(RiemannGP, name))
        assert list(sig.parameters) == ["self", "num_samples", "seed", "observed", "noisy", "tol", "method"]
        assert sig.parameters["num_samples"].default == 64 and sig.parameters["method"].default == "rao-blackwell"
