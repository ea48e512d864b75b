"""The Laplace evidence on the MI355X (mgp_laplace_evidence_site and mgp_scale_rows in csrc/laplace.hip,
manifold_gp_amd/evidence.py): the two kernels against float64 on the same float32 inputs, logdet B by Lanczos quadrature against
the float64 quadrature with the same probes and by the m x m Cholesky against the dense value, the evidence and its
hyper-parameter gradient against the dense float64 restatement (tests/_evidence_ref.py), the training loop and the model
method."""
import warnings

import numpy as np
import pytest
import torch

import _evidence_ref as eref
import _observed_ref as oref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

SITE_GRID_CAP, SITE_PER_STEP = 1024, 256 * 4            # the kernel's grid cap (csrc/laplace.hip): workgroups x nodes per step
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1025, 1546, SITE_GRID_CAP * SITE_PER_STEP + 3 * SITE_PER_STEP + 5]
MEAN = {"poisson": 0.75, "binomial": -0.25, "bernoulli": 0.0}
BIG = 2.0 ** 24
EXTREME = [(f, y) for f in (1e4, -1e4, 88.0, -90.0, 0.0) for y in (0.0, 1.0, BIG)]      # the pairs of test_gpu_counts.py
FLOOR = 1e-6                                            # masks |eta| > 13.8 (Bernoulli, binomial / N) and eta < -13.8 (Poisson)
# The bars of the Lanczos comparison with the float64 quadrature on the same probes: 4 x the worst value measured on the MI355X
# with solve_tol = 1e-6 over the four cases (docs/kernels/evidence.md), never looser than 1e-3.  Value, |difference| / logdet B,
# measured 3.9e-8, 2.1e-8, 1.1e-8, 1.16e-7.  Standard error, |difference| / se, measured 9.2e-8, 7.3e-8, 6.6e-8, 1.81e-6: the se
# of k50_noloop, nu = 3 is 4.5e-4 of logdet B, so the probes' rounding weighs 2000 x more in it than in the mean; it cannot meet
# the value's bar and has its own, derived the same way.
SLQ_BAR = 4 * 1.16e-7
SLQ_SE_BAR = 4 * 1.81e-6
# |device - dense float64| / logdet B of method "dense": 10 x the worst of the five cases measured (4.8e-9, 5.1e-9, 1.4e-8, 1.3e-8,
# 4.6e-9), never looser than 1e-3
DENSE_BAR = 10 * 1.43e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mgp():
    import manifold_gp_amd
    from manifold_gp_amd import _lib
    _lib.lib()
    return manifold_gp_amd


# ------------------------------------------------------------------------------------------------ 1: the site kernel
def _site_inputs(family, n, seed, extremes, frac=0.1):
    """f with eta = f + mean (+ aux) uniform in [-30, 12]; a fraction `frac` observed; latent variances in [0.01, 9]; the 15
    (f, y) pairs of EXTREME at random observed nodes (n >= 63)."""
    rng = np.random.default_rng(seed)
    eta = rng.uniform(-30.0, 12.0, n)
    obs = rng.random(n) < frac
    obs[0] = True
    var = rng.uniform(0.01, 9.0, n)
    if family == "poisson":
        aux = np.log(rng.uniform(0.5, 20.0, n)).astype(np.float32)
        y = rng.choice([0.0, 1.0, 2.0, 5.0, 40.0, 1000.0, BIG], n)
        f = (eta - MEAN[family] - aux).astype(np.float32)
    elif family == "binomial":
        aux = np.where(rng.random(n) < 0.1, BIG, rng.integers(1, 40, n)).astype(np.float32)
        y = np.floor(rng.random(n) * (aux.astype(np.float64) + 1.0)).clip(0.0, aux)
        f = (eta - MEAN[family]).astype(np.float32)
    else:
        aux, y, f = None, (rng.random(n) < 0.5).astype(np.float64), eta.astype(np.float32)
    y = y.astype(np.float32)
    if extremes and n >= 63:
        at = rng.choice(n, len(EXTREME), replace=False)
        f[at] = [e[0] for e in EXTREME]
        y[at] = [e[1] for e in EXTREME]
        obs[at] = True
        if aux is not None:
            aux[at] = 0.0 if family == "poisson" else BIG
    return f, y, aux, obs, var


def _ulps(got, want):
    with np.errstate(over="ignore"):
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _nan_outside(a, obs, dtype=np.float32):
    return a if obs is None or a is None else np.where(obs, a, np.nan).astype(dtype)


def _check_site(dev, family, f, y, aux, obs, var, label, pad=False, h_floor=FLOOR):
    from manifold_gp_amd.evidence import evidence_site
    up = (lambda a: T(np.concatenate([a[:1], a]), dev)[1:]) if pad else (lambda a: T(a, dev))
    opt = lambda a, dt=np.float32: None if a is None else up(_nan_outside(a, obs, dt))     # NaN wherever the node is unobserved
    args = (up(f), opt(y), opt(aux), None if obs is None else up(obs), opt(var, np.float64))
    if pad:
        assert args[0].data_ptr() % 16 == 4 and (var is None or args[4].data_ptr() % 16 == 8)
    root, corr, sums = evidence_site(*args, MEAN[family], family, h_floor)
    want_root, want_corr, want_sums, scale, eff = eref.site_outputs(family, f, y, aux, obs, var, MEAN[family], h_floor)
    gr, gs = root.cpu().numpy(), sums.cpu().numpy()
    assert root.dtype == torch.float32 and sums.dtype == torch.float64 and np.isfinite(gr).all() and np.isfinite(gs).all()
    ur = _ulps(gr, want_root).max()
    assert ur <= 1.0, (label, ur)
    assert (gr[~eff] == 0).all() and (gr[eff] > 0).all()
    assert gs[1] == float(eff.sum()), (label, gs[1], eff.sum())                              # m is exact
    uc = 0.0
    if var is None:
        assert corr is None and gs[2] == 0.0 and gs[3] == 0.0
    else:
        gc = corr.cpu().numpy()
        assert corr.dtype == torch.float32 and np.isfinite(gc).all() and (gc[~eff] == 0).all()
        uc = _ulps(gc, want_corr).max()
        assert uc <= 1.0, (label, uc)
    err = np.abs(gs - want_sums) / np.where(scale > 0, scale, 1.0)
    print("%s %s: root_h %.2f ulp, corr %.2f ulp, sums %.1e %.1e %.1e, m = %d of %d observed, %d nodes"
          % (family, label, ur, uc, err[0], err[2], err[3], eff.sum(), len(f) if obs is None else obs.sum(), len(f)))
    assert err[0] <= 1e-12 and err[2] <= 1e-12 and err[3] <= 1e-14, (label, err)
    root2, corr2, sums2 = evidence_site(*args, MEAN[family], family, h_floor)
    assert torch.equal(root, root2) and torch.equal(sums, sums2) and (corr is None or torch.equal(corr, corr2))   # bitwise
    return int(eff.sum()), int(len(f) if obs is None else obs.sum())


@pytest.mark.parametrize("family", eref.FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_site_kernel_matches_float64(dev, mgp, n, family):
    """root_h and corr within 1 float32 ulp of the rounded float64 reference, 0 off the nodes kept; sum l and sum corr within
    1e-12 of the sum of their absolute terms, max |corr| within 1e-14, m exact; NaN in y, aux and var at unobserved nodes; a
    second call bitwise equal.  10 % observed with the extreme points, every node observed, var NULL; h_floor = 1e-6 masks a
    part of the observed nodes.  The last n runs the grid-stride loop past the grid cap."""
    f, y, aux, obs, var = _site_inputs(family, n, n, extremes=True)
    kept, seen = _check_site(dev, family, f, y, aux, obs, var, "n = %d, 10 %% observed, extremes" % n)
    if n >= 63:
        assert 0 < kept < seen                                                                # the floor masks some, not all
    f, y, aux, obs, var = _site_inputs(family, n, n + 1, extremes=False)
    _check_site(dev, family, f, y, aux, None, var, "n = %d, every node" % n)
    _check_site(dev, family, f, y, aux, obs, None, "n = %d, var NULL" % n)
    if family == "poisson":
        _check_site(dev, family, f, y, None, obs, var, "n = %d, aux NULL" % n)


@pytest.mark.parametrize("family", eref.FAMILIES)
def test_site_kernel_unaligned_arrays_and_the_default_floor(dev, mgp, family):
    """Arrays one float (var: one double) off a 16-byte boundary take the scalar path: the same bounds and the same outputs bit
    for bit as the aligned call.  Then the default floor H_FLOOR = 1e-30."""
    from manifold_gp_amd.evidence import evidence_site
    n = 257
    f, y, aux, obs, var = _site_inputs(family, n, 5, extremes=True)
    _check_site(dev, family, f, y, aux, obs, var, "n = 257, one element off", pad=True)
    pad = lambda a: None if a is None else T(np.concatenate([a[:1], a]), dev)[1:]
    up = lambda a: None if a is None else T(a, dev)
    got = evidence_site(pad(f), pad(y), pad(aux), pad(obs), pad(var), MEAN[family], family, FLOOR)
    want = evidence_site(up(f), up(y), up(aux), up(obs), up(var), MEAN[family], family, FLOOR)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    kept, seen = _check_site(dev, family, f, y, aux, obs, var, "n = 257, default floor", h_floor=eref.H_FLOOR)
    assert kept < seen                                                                        # |eta| = 1e4 stays masked


def test_site_kernel_argument_errors(dev, mgp):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n = 64
    f = torch.zeros(n, device=dev)
    var = torch.ones(n, dtype=torch.float64, device=dev)
    root, corr = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    work = torch.zeros(64, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def call(f_=f, aux_=f, root_=root, sums_=sums, n_=n, family=0, floor=1e-30, work_=work, wb=64, corr_=corr):
        return lib.mgp_laplace_evidence_site(p(f_), p(f), p(aux_), None, p(var), n_, 0.0, family, floor, p(root_), p(corr_), p(sums_),
                                             p(work_), wb, st)
    assert call(f_=None) == -1 and call(root_=None) == -1 and call(sums_=None) == -1 and call(n_=0) == -1 and call(floor=-1.0) == -1
    assert call(family=3) == -3 and call(work_=None) == -2 and call(wb=8) == -2 and call(family=1, aux_=None) == -1
    torch.cuda.synchronize()
    assert bool((root == 7.0).all()) and bool((corr == 7.0).all()) and not sums.any()        # nothing was launched
    assert call(corr_=None) == 0
    torch.cuda.synchronize()
    assert bool((corr == 7.0).all()) and float(sums[2]) == 0.0 and float(sums[1]) == n        # corr NULL: not written
    assert call() == 0 and call(aux_=None) == 0 and call(family=2, aux_=None) == 0


# ------------------------------------------------------------------------------------------------ 2: scale_rows
@pytest.mark.parametrize("P", [1, 3, 4, 12, 16, 17, 256])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1546])
def test_scale_rows_is_the_once_rounded_product(dev, mgp, n, P):
    """s V and fmaf(s, X, V) bitwise equal to s x + v rounded once to float32 (the exact value formed in extended precision: the
    product of two float32 is exact in float64); out a fresh tensor, V itself and X itself; views one float off a 16-byte
    boundary (the scalar path at P % 4 == 0)."""
    from manifold_gp_amd.evidence import scale_rows
    rng = np.random.default_rng(1000 * n + P)
    s = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)
    V, X = rng.standard_normal((n, P)).astype(np.float32), (rng.standard_normal((n, P)) * 3.0).astype(np.float32)
    ext = lambda a: a.astype(np.longdouble)
    want_scale = (ext(s)[:, None] * ext(V)).astype(np.float32)
    want_fma = (ext(s)[:, None] * ext(X) + ext(V)).astype(np.float32)
    sd = T(s, dev)
    off = lambda a: T(np.concatenate([np.zeros(1, np.float32), a.reshape(-1)]), dev)[1:].view(n, P)
    for make in (lambda a: T(a, dev), off):
        Vd, Xd = make(V), make(X)
        assert np.array_equal(scale_rows(sd, Vd).cpu().numpy(), want_scale)
        assert np.array_equal(scale_rows(sd, Vd, Xd).cpu().numpy(), want_fma)
        assert torch.equal(Vd.cpu(), torch.from_numpy(V)) and torch.equal(Xd.cpu(), torch.from_numpy(X))     # inputs untouched
        Xa = make(X)
        assert scale_rows(sd, Vd, Xa, out=Xa) is Xa and np.array_equal(Xa.cpu().numpy(), want_fma)           # out aliases X
        Va = make(V)
        assert scale_rows(sd, Va, Xd, out=Va) is Va and np.array_equal(Va.cpu().numpy(), want_fma)           # out aliases V
        Va = make(V)
        assert np.array_equal(scale_rows(sd, Va, out=Va).cpu().numpy(), want_scale)


# ------------------------------------------------------------------------------------------------ 3-7: the estimators
_PROBLEMS = {}


def _problem(mgp, golden, dev, case, norm, nu, family):
    """One problem per (fixture, normalisation, nu, family), built once: the descriptor scaled to a prior marginal variance of about
    9, the dense float64 matrix the kernels apply, the family's data, the device's fit, and at the device's mode the float64 site
    values and the dense evidence."""
    key = (case, norm, nu)
    if key not in _PROBLEMS:
        g = golden(case)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = oref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        _PROBLEMS[key] = dict(g=g, desc=d1.with_(scale=scale), Q=scale * Q1, scale=scale)
    base = _PROBLEMS[key]
    if family not in base:
        d = eref.data(base["g"], family)
        nan = lambda a: T(np.where(d["obs"], a, np.nan).astype(np.float32), dev)
        obs = T(d["obs"], dev)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
            if family == "bernoulli":
                from manifold_gp_amd.classification import laplace_fit
                fit = laplace_fit(base["desc"], nan(d["y"]), obs)
            else:
                from manifold_gp_amd.counts import laplace_fit_counts
                c = eref.cref.counts(base["g"])
                kw = dict(exposure=T(c["E"], dev)) if family == "poisson" else dict(trials=nan(c["N"]))
                fit = laplace_fit_counts(base["desc"], nan(d["y"]), obs, family=family, **kw)
        assert fit.converged
        f = fit.mean.double().cpu().numpy()
        _, h, hp = eref.site(family, f, d["y"], d["aux"], d["obs"], d["mean"])
        eff = d["obs"] & (h >= eref.H_FLOOR)
        base[family] = dict(base, d=d, fit=fit, f=f, h=h, hp=hp, eff=eff, m=int(eff.sum()), z=eref.log_z(base["Q"], f, d))
    return base[family]


def _root_h(p, dev):
    from manifold_gp_amd.evidence import evidence_site
    fit = p["fit"]
    fam = p["d"]["family"]
    root, _, sums = evidence_site(fit.mean, fit.y, getattr(fit, "_aux", None), fit.observed, None, p["d"]["mean"], fam)
    assert int(sums[1]) == p["m"]
    return root


@pytest.mark.parametrize("case, norm, nu", eref.SLQ_CASES)
def test_logdet_b_slq_matches_the_float64_quadrature_with_the_same_probes(mgp, golden, dev, case, norm, nu):
    """method "slq" with the probes given, 16 probes and 12 steps, against oracle.solvers.slq_logdet_same_probes on the dense B of
    the matrix the kernels apply: value within SLQ_BAR of logdet B, the standard error within SLQ_SE_BAR relative, the estimate
    within 5 of its standard errors of the dense value."""
    from manifold_gp_amd.evidence import logdet_b
    p = _problem(mgp, golden, dev, case, norm, nu, "bernoulli")
    Z = eref.probes(p["eff"], eref.SLQ_PROBES, eref.SLQ_SEED)
    per_ref, want, se_ref = eref.slq_per_probe(eref.b_matmul(p["Q"], p["h"]), Z, eref.SLQ_STEPS, p["m"])
    value, se, per = logdet_b(p["desc"], _root_h(p, dev), p["m"], steps=eref.SLQ_STEPS, solve_tol=1e-6, method="slq",
                              probes=T(Z.astype(np.float32), dev))
    dense = p["z"]["logdet"]
    print("%s %s nu = %d: logdet B dense %.4f, device %.5f +- %.5f, float64 same probes %.5f +- %.5f: |difference| / logdet B = %.2e, "
          "se relative %.2e, worst probe %.2e of logdet B, %.2f standard errors from dense"
          % (case, norm, nu, dense, value, se, want, se_ref, abs(value - want) / dense, abs(se - se_ref) / se_ref,
             np.abs(per - per_ref).max() / dense, abs(value - dense) / se))
    assert per.shape == (eref.SLQ_PROBES,)
    assert abs(value - want) <= SLQ_BAR * dense
    assert abs(se - se_ref) <= SLQ_SE_BAR * se_ref
    assert abs(value - dense) <= 5.0 * se
    # the default probes are those of the restatement: the same call without probes= (the solver's tolerance split may have
    # adapted in between, so not bitwise)
    again = logdet_b(p["desc"], _root_h(p, dev), p["m"], num_probes=eref.SLQ_PROBES, steps=eref.SLQ_STEPS, seed=eref.SLQ_SEED,
                     method="slq")
    print("    default probes: |difference| / logdet B = %.2e, se relative %.2e" % (abs(again[0] - want) / dense, abs(again[1] - se_ref) / se_ref))
    assert abs(again[0] - want) <= SLQ_BAR * dense and abs(again[1] - se_ref) <= SLQ_SE_BAR * se_ref


DENSE_CASES = [("dumbbell_k10_loop", "symmetric", 2, "bernoulli"), ("dumbbell_k10_loop", "symmetric", 2, "poisson"),
               ("dumbbell_k10_loop", "symmetric", 2, "binomial"), ("dumbbell_k10_loop", "randomwalk", 3, "bernoulli"),
               ("dumbbell_k50_noloop", "symmetric", 1, "bernoulli")]


@pytest.mark.parametrize("case, norm, nu, family", DENSE_CASES)
def test_dense_logdet_and_the_evidence_value(mgp, golden, dev, case, norm, nu, family):
    """method "dense" against the dense float64 logdet B at the device's mode within DENSE_BAR relative; "auto" picks it at m = 149;
    the evidence's log-likelihood and quadratic part within 1e-6 relative of the restatement's, the value within the sum of the
    three bounds."""
    from manifold_gp_amd.evidence import logdet_b
    p = _problem(mgp, golden, dev, case, norm, nu, family)
    z = p["z"]
    value, se, per = logdet_b(p["desc"], _root_h(p, dev), p["m"], method="dense")
    ev = p["fit"].evidence()
    e_ld, e_ll, e_q = abs(value - z["logdet"]) / z["logdet"], abs(ev.log_likelihood - z["log_likelihood"]) / abs(z["log_likelihood"]), \
        abs(ev.quad - z["quad"]) / z["quad"]
    print("%s %s nu = %d %s: m = %d, logdet B dense %.5f, device %.5f (relative %.2e); log Z %.5f, device %.5f; log-likelihood "
          "relative %.1e, quad relative %.1e" % (case, norm, nu, family, p["m"], z["logdet"], value, e_ld, z["value"], float(ev.value),
                                                 e_ll, e_q))
    assert se == 0.0 and per is None and e_ld <= DENSE_BAR
    assert p["m"] <= 512 and ev.method == "dense" and ev.m == p["m"] and ev.se == 0.0
    assert abs(ev.logdet - z["logdet"]) <= DENSE_BAR * z["logdet"]
    assert ev.value.dtype == torch.float64 and ev.value.shape == () and not ev.value.requires_grad and ev.solves is None
    assert e_ll <= 1e-6 and e_q <= 1e-6
    # the site kernel's own sum of l, plus the family's constant, is the fit's log-likelihood: two float64 sums of the same
    # terms, each within the sibling kernels' 1e-12 of the sum of their absolute values
    l_abs = np.abs(eref.site(family, p["f"], p["d"]["y"], p["d"]["aux"], p["d"]["obs"], p["d"]["mean"])[0]).sum()
    assert abs(ev.site_sums[0] + p["d"]["const"] - ev.log_likelihood) <= 2e-12 * l_abs + 4 * np.spacing(abs(ev.log_likelihood))
    assert ev.site_sums[1] == p["m"] and ev.site_sums[2] == 0.0 and ev.site_sums[3] == 0.0
    assert abs(float(ev.value) - z["value"]) <= 1e-6 * (abs(z["log_likelihood"]) + z["quad"]) + 0.5 * DENSE_BAR * z["logdet"]
    assert float(ev.value) == ev.log_likelihood - ev.quad - 0.5 * ev.logdet
    if family == "bernoulli":
        slq = p["fit"].evidence(method="slq")
        print("    method slq: log Z %.4f +- %.4f" % (float(slq.value), slq.se))
        assert slq.method == "slq" and slq.se == 0.5 * slq.logdet_se and abs(float(slq.value) - z["value"]) <= 5.0 * slq.se + 1e-3 * abs(z["value"])


def check_theta(got, ref, scale, names):
    """The operator-level bound of test_gpu_gradients.py: |got - ref| <= 2e-4 scale; where |ref| >= scale / 10 also <= 2e-3 |ref|."""
    worst = 0.0
    for nm, x, r, s in zip(names, got, ref, scale):
        assert abs(x - r) <= 2e-4 * s, (nm, x, r, s)
        if abs(r) >= 0.1 * s:
            assert abs(x - r) <= 2e-3 * abs(r), (nm, x, r)
        worst = max(worst, abs(x - r) / (2e-4 * s))
    return worst


def _rel_residual(A, X, B):
    """the largest float64 true relative residual over the columns"""
    return float((np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)).max())


@pytest.mark.parametrize("family", ["bernoulli", "poisson"])
def test_gradient_matches_float64_bilinear_forms(mgp, golden, dev, family):
    """k10_loop, symmetric, nu = 2, given probes and variance = the dense diag(A^-1): the gradients of the evidence with respect
    to graph bandwidth, length scale and output scale against the float64 derivatives of the three bilinear forms on the
    device's own u, X, Y and mode (oracle/grad_ref.py), within the operator-level bar of test_gpu_gradients.py; the float64 true
    residuals of the u, X and Y solves <= 2 tol (u and X are the float64 solutions of the refined solves, which is what the
    bilinear forms use: rounded to float32, X alone would leave 2.4e-6 to 2.6e-6 at tol = 1e-6); and the same surrogate with exact
    float64 solves within 5 standard errors of the probe term of the dense analytic gradient (output scale and length scale)."""
    from oracle.grad_ref import bilinear_grads_f64
    O = mgp.operators
    case, norm, nu, tol = "dumbbell_k10_loop", "symmetric", 2, 1e-6
    p = _problem(mgp, golden, dev, case, norm, nu, family)
    g, d, n, Q = p["g"], p["d"], p["desc"].n, p["Q"]
    theta = [float(np.float32(v)) for v in (float(g["eps"]), float(g["kappa"]), p["scale"])]
    th = [torch.tensor(v, device=dev, requires_grad=True) for v in theta]
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    lap = O.GraphLaplacianOperator(val, idx, n, th[0].view(1, 1), norm, bool(g["self_loops"]))
    op = O.ScaleWrapperOperator(O.PrecisionMaternOperator(lap, nu, th[1]), th[2])
    A = Q + np.diag(p["h"])
    var = np.diag(np.linalg.inv(A))
    P = eref.SLQ_PROBES
    Z = eref.probes(p["eff"], P, 4321)
    ev = p["fit"].evidence(operator=op, variance=T(var, dev), probes=T(Z.astype(np.float32), dev), solve_tol=tol)
    assert ev.value.requires_grad and ev.method == "dense"
    got = [float(x) for x in torch.autograd.grad(ev.value, th)]
    s = {k: (v.double().cpu().numpy() if torch.is_tensor(v) else v) for k, v in ev.solves.items()}
    f, u, X, Y = p["f"], s["u"], s["X"], s["Y"]
    V = np.concatenate([f[:, None], Y], 1)
    W = np.concatenate([0.5 * (u - f)[:, None], X * (0.5 / P)], 1)
    val64, idx64 = torch.from_numpy(g["edge_value"].astype(np.float64)), torch.from_numpy(g["edge_index"].astype(np.int64))
    ref, scale = bilinear_grads_f64(val64, idx64, n, theta + [0.0], nu, norm, bool(g["self_loops"]), V, W, stop="Q2")
    worst = check_theta(got, ref[:3], scale[:3], ["eps", "kappa", "outputscale"])
    # the solves: float64 true residuals on the matrix the kernels apply, with the weights the device used
    SZ = s["root_h"][:, None] * s["Z"]
    Adev = Q + np.diag(s["w"] / s["s_ref"])
    assert ev.solves["X"].dtype == torch.float64 and ev.solves["u"].dtype == torch.float64 and ev.solves["Y"].dtype == torch.float32
    rx, ry, ru = _rel_residual(Q, X, SZ), _rel_residual(Adev, Y, SZ), _rel_residual(Adev, u[:, None], s["corr"][:, None])
    rx32 = _rel_residual(Q, X.astype(np.float32).astype(np.float64), SZ)
    # exact solves with the same probes against the dense analytic gradient
    stat = []
    for name, dQ in (("outputscale", Q / p["scale"]),
                     ("kappa", -2.0 * nu * (2.0 * nu / theta[1] ** 2) / theta[1] * p["scale"] * _a_power(p, nu, theta[1]))):
        exact, _ = eref.gradient(Q, dQ, f, d)
        est, se = eref.probe_gradient(Q, dQ, f, d, Z)
        stat.append((name, exact, est, se))
    print("%s: gradient (eps, kappa, outputscale) device %s, float64 on the device's vectors %s, worst %.4f of the bound; true "
          "residuals X %.2e (rounded to float32: %.2e), Y %.2e, u %.2e; exact solves: %s"
          % (family, ["%.6f" % v for v in got], ["%.6f" % v for v in ref[:3]], worst, rx, rx32, ry, ru,
             ["%s: dense %.4f, probes %.4f +- %.4f" % t for t in stat]))
    assert max(rx, ry, ru) <= 2.0 * tol
    for name, exact, est, se in stat:
        assert abs(est - exact) <= 5.0 * se, (name, exact, est, se)


def _a_power(p, nu, kappa):
    """(tau I + L_sym)^(nu - 1) of the device's matrix (symmetric normalisation): Q / scale = A^nu, so A = (Q / scale)^(1 / nu)
    by its eigendecomposition"""
    w, U = np.linalg.eigh(p["Q"] / p["scale"])
    return (U * np.maximum(w, 0.0) ** ((nu - 1.0) / nu)) @ U.T


def test_laplace_train_raises_the_dense_evidence(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, Bernoulli, Adam(0.1) on the raw length scale and output scale from _evidence_ref.TRAIN (the
    fixture's length scale at a prior variance of 9): the dense float64 log Z at the device run's end hyper-parameters exceeds
    the one at its start by at least half the gain of the float64 run of the same optimiser with exact gradients, 12.906 in 10
    steps (test_evidence_cpu.py reruns it).  Measured on the MI355X: gains of 12.928, 12.954 and 13.005 (the variance seed is drawn)."""
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.utils import laplace_train
    TRAIN_KAPPA0, TRAIN_SCALE0, TRAIN_STEPS, TRAIN_LR, gain64 = (eref.TRAIN[k] for k in ("kappa0", "scale0", "steps", "lr", "gain_f64"))
    case, norm, nu = "dumbbell_k10_loop", "symmetric", 2
    g = golden(case)
    d = eref.data(g, "bernoulli")
    assert gain64 >= 5.0
    x = T(g["train_x"], dev)
    y, obs = T(np.where(d["obs"], d["y"], np.nan).astype(np.float32), dev), T(d["obs"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization=norm, num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=TRAIN_KAPPA0)
    model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, TRAIN_SCALE0).to(dev)).to(dev)
    kern.raw_graphbandwidth.requires_grad_(False)
    opt = torch.optim.Adam([kern.raw_lengthscale, model.covar_module.raw_outputscale], lr=TRAIN_LR)
    kappa0, scale0 = float(kern.lengthscale), float(model.covar_module.outputscale)
    last = laplace_train(model, opt, observed=obs, max_iter=TRAIN_STEPS - 1, tolerance=0.0, evidence_kw=dict(var_samples=64))
    kappa1, scale1 = float(kern.lengthscale), float(model.covar_module.outputscale)

    def dense(kappa, scale):
        Q = eref.dense_q(g, norm, nu, float(g["eps"]), kappa, scale).numpy()
        return eref.log_z(Q, eref.mode(Q, d), d)["value"]
    z0, z1 = dense(kappa0, scale0), dense(kappa1, scale1)
    print("laplace_train: float64 run gains %.3f; device run %.4f -> %.4f (gain %.3f; kappa %.4f -> %.4f, scale %.5g -> %.5g), last "
          "loss %.5f" % (gain64, z0, z1, z1 - z0, kappa0, kappa1, scale0, scale1, last))
    assert abs(kappa0 - TRAIN_KAPPA0) <= 1e-6 * TRAIN_KAPPA0 and abs(scale0 - TRAIN_SCALE0) <= 1e-5 * TRAIN_SCALE0
    assert np.isfinite(last)
    assert z1 - z0 >= 0.5 * gain64


def test_model_method_agrees_with_the_fit(mgp, golden, dev):
    from manifold_gp_amd.evidence import LaplaceEvidence
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    g = golden("dumbbell_k10_loop")
    d = eref.data(g, "bernoulli")
    x = T(g["train_x"], dev)
    y, obs = T(np.where(d["obs"], d["y"], np.nan).astype(np.float32), dev), T(d["obs"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="symmetric",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    model = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 1.1e-5).to(dev)).to(dev)
    c = model.laplace_evidence(observed=obs, method="slq", seed=11)                           # the parameters require grad
    assert c.value.requires_grad and c.solves is not None
    with torch.no_grad():
        a = model.laplace_evidence(observed=obs, method="slq", seed=11, rtol=1e-5)
    b = model.laplace_posterior(observed=obs, rtol=1e-5).evidence(method="slq", seed=11)
    assert isinstance(a, LaplaceEvidence) and a.method == "slq" and a.se > 0.0 and not a.value.requires_grad
    assert torch.equal(a.value, b.value) and a.logdet == b.logdet and a.se == b.se and np.array_equal(a.per_probe, b.per_probe)
    assert abs(float(c.value) - float(a.value)) <= 1e-3 * abs(float(a.value))                 # the surrogate adds exactly 0
    # max_iter belongs to both signatures and goes to the fit; fit_kw / evidence_kw name the receiver
    with torch.no_grad():
        e = model.laplace_evidence(observed=obs, method="slq", seed=11, max_iter=4000, fit_kw=dict(rtol=1e-5), evidence_kw=dict(max_iter=3000))
        assert abs(float(e.value) - float(a.value)) <= 1e-6 * abs(float(a.value))
        with pytest.raises(TypeError):
            model.laplace_evidence(observed=obs, evidence_kw=dict(rtol=1e-5))
    with pytest.raises(ValueError, match="family"):
        model.laplace_evidence(observed=obs, family="gauss")
    with pytest.raises(NotImplementedError):
        model.laplace_posterior_multiclass(2, observed=obs).evidence()
