"""Count fits, host side (no GPU): the float64 restatement the GPU tests are checked against (tests/_counts_ref.py) is itself
checked -- its mode is stationary, its gradient and curvature agree with central differences, its outputs are finite at
extreme latents --, the C-ABI and Python argument checks, and the stopping rule of the fit (classification._newton with
step_tol) on a dense simulation whose vectors are rounded to float32 where the device's are."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

import _counts_ref as cref
import _observed_ref as oref

FAMILIES = ["poisson", "binomial"]
_Q = {}


def _precision(golden, case, norm, nu):
    """The fixture's precision scaled to a prior marginal variance of about 9, as test_laplace_cpu.py::problem does."""
    key = (case, norm, nu)
    if key not in _Q:
        g = golden(case)
        Q1, _ = oref.precision_root(oref.oracle(g, norm), nu, float(g["kappa"]), 1.0, norm)
        _Q[key] = (np.diag(np.linalg.inv(Q1)).mean() / 9.0) * Q1
    return _Q[key]


def _data(golden, case, family):
    c = cref.counts(golden(case))
    return cref.poisson_data(c) if family == "poisson" else cref.binomial_data(c)


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_mode_is_stationary_and_psi_monotone(golden, family):
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    d = _data(golden, "dumbbell_k10_loop", family)
    f, trace = cref.newton(Q, d)
    res = np.abs(cref.gradient(Q, f, d)).max()
    g0 = np.abs(cref.gradient(Q, np.zeros_like(f), d)).max()
    print("%s: max |g - Q f| = %.2e after %d steps (max |g(0)| = %.1f, largest count %d, mean %.3f, s_ref %g); max |f| = %.2f"
          % (family, res, len(trace), g0, d["y"][d["obs"]].max(), d["mean"], d["s_ref"], np.abs(f).max()))
    assert res <= 1e-10
    assert np.abs(f).max() > 1.0                                   # a non-linear regime
    psis = [cref.psi(Q, np.zeros_like(f), d)] + [t[0] for t in trace]
    assert all(b >= a - 1e-12 * abs(a) for a, b in zip(psis, psis[1:]))


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_gradient_and_curvature_match_central_differences(golden, family):
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    d = _data(golden, "dumbbell_k10_loop", family)
    rng = np.random.default_rng(3)
    f = 0.5 * rng.standard_normal(Q.shape[0])
    grad = cref.gradient(Q, f, d)
    eps = 1e-5
    obs = d["obs"]
    for i in list(np.flatnonzero(obs)[:5]) + list(np.flatnonzero(~obs)[:5]):
        e = np.zeros_like(f)
        e[i] = eps
        fd = (cref.psi(Q, f + e, d) - cref.psi(Q, f - e, d)) / (2 * eps)
        # psi is a sum of size |psi|: its central difference carries |psi| 2^-52 / eps of rounding
        assert abs(fd - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])) + 4 * 2.0 ** -52 * abs(cref.psi(Q, f, d)) / eps, (i, fd, grad[i])
    args = (d["y"], d["aux"], obs, d["mean"])
    g_plus, g_minus = cref.site(family, f + eps, *args)[1], cref.site(family, f - eps, *args)[1]
    h = cref.site(family, f, *args)[2]
    assert (np.abs(-(g_plus - g_minus) / (2 * eps) - h) <= 1e-8 * np.maximum(1.0, h)).all()
    l_plus, l_minus = cref.site(family, f + eps, *args)[0], cref.site(family, f - eps, *args)[0]
    g = cref.site(family, f, *args)[1]
    assert (np.abs((l_plus - l_minus) / (2 * eps) - g) <= 1e-6 * np.maximum(1.0, np.abs(g))).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_site_is_finite_at_extreme_latents(family):
    fs, ys = [1e4, -1e4, 88.0, -90.0, 0.0], [0.0, 1.0, 2.0 ** 24]
    f = np.repeat(fs, len(ys)).astype(np.float32)
    y = np.tile(ys, len(fs)).astype(np.float32)
    aux = None if family == "poisson" else np.full(f.shape, 2.0 ** 24, np.float32)
    qf = np.linspace(-2.0, 2.0, f.shape[0]).astype(np.float32)
    w, rhs, sums, _, _ = cref.site_outputs(family, f, qf, y, aux, None, 2.0 ** -24, 0.0)
    assert np.isfinite(w).all() and np.isfinite(rhs).all() and np.isfinite(sums[:3]).all()
    if family == "poisson":
        assert (w[:3] == cref.FLT_MAX).all() and (rhs[:3] == -cref.FLT_MAX).all()      # mu = e^700: saturated, not inf
        assert (w[3:6] == 0).all() and np.isinf(sums[3])
        assert w[-1] == np.float32(2.0 ** -24) and rhs[-1] == np.float32(1.0 - 2.0 ** -24 - 2.0 ** -24 * 2.0)
    else:
        assert (w[:6] == 0).all() and w[-1] == 0.25 and np.isfinite(sums[3])
        assert rhs[2] == np.float32(2.0 ** -24 * -qf[2].astype(np.float64))                 # y = N at eta = 1e4: g = 0
        assert abs(sums[0] - cref.site(family, f, y, aux, None, 0.0)[0].sum()) == 0.0
        assert cref.site(family, f, y, aux, None, 0.0)[0][0] == -2.0 ** 24 * 1e4             # 0 of 2^24 at eta = 1e4


# ------------------------------------------------------------------------------------------------ host-side checks
def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mgp_count_site_workspace_bytes", "mgp_count_site"):
        assert name in _lib.SIGNATURES
        assert hasattr(handle, name)


def test_entry_points_check_their_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 8)()
    dbl = (ctypes.c_double * 8)()
    u, d = ctypes.addressof(buf), ctypes.addressof(dbl)
    assert lib.mgp_count_site_workspace_bytes(0) == 0
    assert lib.mgp_count_site_workspace_bytes(1) == 32 and lib.mgp_count_site_workspace_bytes(1025) == 64
    assert lib.mgp_count_site_workspace_bytes(2 ** 40) == 1024 * 32                 # the grid cap
    assert lib.mgp_bernoulli_site_workspace_bytes(1025) == 64                       # unchanged
    site = lib.mgp_count_site
    for fam in (0, 1):
        assert site(None, None, u, u, None, 4, 1.0, 0.0, fam, u, u, d, d, 64, None) == -1
        assert site(u, None, None, u, None, 4, 1.0, 0.0, fam, u, u, d, d, 64, None) == -1
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, None, u, d, d, 64, None) == -1
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, u, None, d, d, 64, None) == -1
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, u, u, None, d, 64, None) == -1
        assert site(u, None, u, u, None, 0, 1.0, 0.0, fam, u, u, d, d, 64, None) == -1
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, u, u, d, None, 64, None) == -2
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, u, u, d, d, 31, None) == -2
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, u, u, d, d + 4, 64, None) == -2      # misaligned
    assert site(u, None, u, None, None, 4, 1.0, 0.0, 1, u, u, d, d, 64, None) == -1             # binomial without trials
    for fam in (2, -1, 7):
        assert site(u, None, u, u, None, 4, 1.0, 0.0, fam, u, u, d, d, 64, None) == -3


def _fake_desc(nu=2, form=0):
    from manifold_gp_amd.operators._descriptor import Descriptor
    sq = torch.ones(3)
    data = types.SimpleNamespace(dsqrt=sq, dinvsqrt=sq, graph=types.SimpleNamespace(n=3, device=torch.device("cpu")))
    return Descriptor(data=data, nu=nu, kappa=1.0, form=form, noise=0.1 if form else 0.0)


def test_laplace_fit_counts_argument_checks():
    from manifold_gp_amd.counts import count_site, laplace_fit_counts as fit
    d = _fake_desc()
    y = torch.tensor([0.0, 3.0, 7.0])
    N = torch.tensor([1.0, 3.0, 9.0])
    some = torch.tensor([True, False, True])
    nan = float("nan")
    for bad in ([0.0, 0.5, 1.0], [0.0, -1.0, 1.0], [0.0, 2.0 ** 24 + 2, 1.0], [nan, 1.0, 1.0]):
        with pytest.raises(ValueError, match="integers in"):
            fit(d, torch.tensor(bad))
    with pytest.raises(ValueError, match="integers in"):
        fit(d, torch.tensor([nan, 1.0, 1.0]), observed=some)                        # NaN at an observed node
    with pytest.raises(ValueError, match="no node"):
        fit(d, y, observed=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError):
        fit(d, y, observed=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError):
        fit(d, y, observed=torch.ones(3))
    with pytest.raises(ValueError):
        fit(d, torch.zeros(4))
    with pytest.raises(ValueError, match="family"):
        fit(d, y, family="negative-binomial")
    with pytest.raises(ValueError, match="f0"):
        fit(d, y, f0=torch.zeros(2))
    for bad in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("inf"), 1.0], [1.0, nan, 1.0]):
        with pytest.raises(ValueError, match="exposure"):
            fit(d, y, exposure=torch.tensor(bad))
    with pytest.raises(ValueError, match="exposure"):
        fit(d, y, exposure=torch.ones(4))
    with pytest.raises(ValueError, match="trials"):
        fit(d, y, trials=N)                                                         # trials with Poisson
    with pytest.raises(ValueError, match="exposure"):
        fit(d, y, family="binomial", trials=N, exposure=torch.ones(3))              # exposure with binomial
    with pytest.raises(ValueError, match="needs trials"):
        fit(d, y, family="binomial")
    for bad in ([1.0, 3.5, 9.0], [0.0, 3.0, 9.0], [1.0, 2.0, 9.0], [1.0, nan, 9.0]):  # not whole, < 1, < y, NaN
        with pytest.raises(ValueError, match="trials"):
            fit(d, y, family="binomial", trials=torch.tensor(bad))
    with pytest.raises(ValueError, match="every observed count is 0"):
        fit(d, torch.zeros(3))
    with pytest.raises(ValueError, match="mean"):
        fit(d, y, mean=float("inf"))
    with pytest.raises(ValueError, match="step_tol"):
        fit(d, y, step_tol=0.0)
    for bad in ("1.0", [1.0], torch.zeros(2), True):
        with pytest.raises(ValueError, match="mean must be a real scalar"):
            fit(d, y, mean=bad)
        with pytest.raises(ValueError, match="step_tol must be a real scalar"):
            fit(d, y, step_tol=bad)
    with pytest.raises(NotImplementedError):
        fit(_fake_desc(form=2), y)
    # valid arguments on host tensors: the checks pass, the first device call refuses
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(d, torch.tensor([0.0, nan, 7.0]), observed=some, exposure=torch.tensor([2.0, nan, 0.5]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(d, torch.zeros(3), mean=-1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(d, torch.tensor([0, 3, 7]), family="binomial", trials=torch.tensor([1, 3, 9]))
    with pytest.raises(ValueError, match="family"):
        count_site(torch.zeros(3), None, y, None, None, 1.0, 0.0, "gauss")
    with pytest.raises(ValueError, match="trials"):
        count_site(torch.zeros(3), None, y, None, None, 1.0, 0.0, "binomial")


def test_defaults_of_mean_and_s_ref():
    from manifold_gp_amd.counts import _validate
    d = _fake_desc()
    some = torch.tensor([True, False, True])
    y = torch.tensor([2.0, 900.0, 6.0])
    *_, mean, s_ref = _validate(d, y, some, "poisson", torch.tensor([1.0, 5.0, 3.0]), None, None, 1e-3, None)
    assert mean == pytest.approx(np.log(8.0 / 4.0), abs=1e-15) and s_ref == 2.0 ** -3          # max observed y = 6
    *_, mean, s_ref = _validate(d, y, None, "poisson", None, None, None, 1e-3, None)
    assert mean == pytest.approx(np.log(908.0 / 3.0), abs=1e-15) and s_ref == 2.0 ** -10
    *_, mean, s_ref = _validate(d, torch.tensor([0.0, 1.0, 1.0]), None, "poisson", None, None, 0.5, 1e-3, None)
    assert mean == 0.5 and s_ref == 1.0
    for half, tol in ((np.float32(0.5), np.float64(1e-3)), (torch.tensor(0.5), torch.tensor([1e-3])), (np.int64(1), 1)):
        *_, mean, _ = _validate(d, y, None, "poisson", None, None, half, tol, None)             # numpy scalars, 0-d tensors
        assert isinstance(mean, float) and mean == float(half)
    *_, mean, s_ref = _validate(d, torch.tensor([0.0, 1.0, 1.0]), None, "binomial", None, torch.ones(3), None, 1e-3, None)
    assert mean == 0.0 and s_ref == 4.0                                                        # the Bernoulli fit's S_REF
    *_, mean, s_ref = _validate(d, y, some, "binomial", None, torch.tensor([16.0, 1.0, 9.0]), None, 1e-3, None)
    assert s_ref == 4.0 / 16.0
    *_, s_ref = _validate(d, y, some, "binomial", None, torch.tensor([17.0, 1.0, 9.0]), 0.25, 1e-3, None)
    assert s_ref == 4.0 / 32.0


def test_model_method_and_exports():
    import manifold_gp_amd
    from manifold_gp_amd.models import RiemannGP
    sig = inspect.signature(RiemannGP.laplace_posterior_counts)
    assert list(sig.parameters) == ["self", "observed", "kw"]
    assert manifold_gp_amd.counts.laplace_fit_counts and issubclass(manifold_gp_amd.counts.CountLaplaceFit,
                                                                   manifold_gp_amd.classification.LaplaceFit)
    sig = inspect.signature(manifold_gp_amd.counts.laplace_fit_counts)
    assert list(sig.parameters) == ["desc", "y", "observed", "family", "exposure", "trials", "mean", "step_tol", "max_newton",
                                    "cg_tol", "max_iter", "f0"]
    assert sig.parameters["step_tol"].default == 1e-3
    newton = inspect.signature(manifold_gp_amd.classification._newton)
    assert newton.parameters["step_tol"].default is None


# ------------------------------------------------------------------------------------------------ the stopping rule
def test_step_rule_is_off_by_default_and_ends_on_a_small_full_step():
    """_newton on a scalar quadratic: with step_tol None it runs to the gradient rule; with step_tol it stops after the first
    accepted full step whose size is <= step_tol, and never on a halved one."""
    from manifold_gp_amd.classification import _newton

    def loop(step_tol, scale):
        # psi = -(f - 1)^2 / 2 (as sums[0]); the 'solver' returns scale x the Newton step
        site = lambda f, qf: (None, 1.0 - f, [-0.5 * float((f - 1.0) ** 2), 0.0, abs(float(1.0 - f)), float((1.0 - f) ** 2)])
        return _newton("t", site, lambda f: None, lambda aux, rhs: (scale * rhs, 0), np.float64(0.0), None, 1e-9, 50,
                       step_tol=step_tol)
    f, _, _, conv, its, hist = loop(None, 0.5)
    assert conv and its == 30 and abs(f - 1.0) <= 1e-9                                # 2^-30 <= 1e-9: the gradient rule
    f, _, _, conv, its, hist = loop(1e-3, 0.5)
    assert conv and its == 10 and hist[-1][2] == 1.0                                  # the step 2^-10 <= 1e-3
    f, _, _, conv, its, hist = loop(1e-3, 2.5)                                        # overshoots: every step is halved
    assert conv and all(h[2] < 1.0 for h in hist) and abs(f - 1.0) <= 1e-9            # ended by the gradient, not the step


CASES = [(c, n, nu) for c in ("dumbbell_k10_loop", "dumbbell_k50_noloop") for n in ("symmetric", "randomwalk") for nu in (1, 2, 3)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case, norm, nu", CASES)
def test_step_rule_reaches_the_mode_in_float32(golden, case, norm, nu, family):
    """From f0 = 0 the float32-rounded iteration with step_tol = 1e-3 converges in <= 10 steps, all full, and lands within 1e-5
    of the float64 mode.  Measured: 7-8 steps (Poisson), 6 (binomial); errors of a few 1e-7."""
    Q = _precision(golden, case, norm, nu)
    d = _data(golden, case, family)
    f64, _ = cref.newton(Q, d)
    f, converged, its, history = cref.simulate(Q, d)
    err = np.abs(f.astype(np.float64) - f64).max()
    rel = np.abs(cref.gradient(Q, f.astype(np.float64), d)).max() / np.abs(cref.gradient(Q, 0.0 * f64, d)).max()
    print("%s %s %s nu = %d: %d steps %s, max |f - f64| = %.2e, relative gradient %.1e, max |f| = %.2f"
          % (family, case, norm, nu, its, [h[2] for h in history], err, rel, np.abs(f64).max()))
    assert converged and its <= 10
    assert all(h[2] == 1.0 for h in history), history
    assert err <= 1e-5, err


@pytest.mark.parametrize("start, first", [(-3.0, [1 / 16, 1 / 2]), (-5.0, [1 / 64, 1 / 8])])
def test_step_rule_from_a_low_start(golden, start, first):
    """Poisson from f0 = start at every node: the rate is far too low, the first Newton steps overshoot (mu grows like e^delta)
    and are halved -- 1/16, 1/2, then full from -3; 1/64, 1/8, then full from -5 -- inside the 10-halving budget."""
    Q = _precision(golden, "dumbbell_k10_loop", "symmetric", 2)
    d = _data(golden, "dumbbell_k10_loop", "poisson")
    f64, _ = cref.newton(Q, d)
    f, converged, its, history = cref.simulate(Q, d, f0=np.full(Q.shape[0], start, np.float32))
    steps = [h[2] for h in history]
    err = np.abs(f.astype(np.float64) - f64).max()
    print("f0 = %g: steps %s, max |f - f64| = %.2e" % (start, steps, err))
    assert converged and err <= 1e-5
    assert steps[:2] == first and all(s == 1.0 for s in steps[2:]), steps
