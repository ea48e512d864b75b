"""The dispersion gradient of the negative-binomial Laplace evidence on the MI355X (mgp_nb_dispersion_sums in csrc/laplace.hip,
evidence.laplace_evidence(dispersion=), DispersionParameter and learn_dispersion of counts.py, the live dispersion of
utils.laplace_train): the kernel against float64 on the same float32 inputs, the gradient of a fit against the dense float64
restatement (tests/_nb_dispersion_ref.py), and the two training loops against their float64 runs."""
import warnings

import numpy as np
import pytest
import torch

import _evidence_ref as eref
import _nb_dispersion_ref as dr
import _nb_ref as nb
import _observed_ref as oref
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

NBF = "negative_binomial"
CASE, NORM, NU = "dumbbell_k10_loop", "symmetric", 2
MEAN = 0.75
BIG = 2.0 ** 24
SIZES = [1, 3, 4, 5, 257, 4099]
CAP_N = 1024 * 256 * 4 + 3 * 256 * 4 + 5                 # 1 051 653: beyond the grid cap, 1024 workgroups x 1024 nodes
KERNEL_R = [2.0 ** -10, 1.5, 2.0 ** 20]
SPECIAL = np.array([0.0, 1e-8, 1.0, 20.0, 40.0, 88.0, 90.0, 200.0, 1e4])
FLOOR = 1e-6                                             # masks the nodes far out in either tail
# a row against the restatement, relative to the sum of its absolute terms: the float64 sums' 1e-12 of the sibling kernels, and
# no less than 4 x the error of psi_diff measured against mpmath on the CPU (test_nb_dispersion_cpu.py)
ROW_BAR = max(1e-12, dr.DEVICE_PSI_ULP * 2.0 ** -53)
# d log Z / dr of a fit at r = 2 against the float64 gradient at the float64 mode, relative to the sum of the absolute terms of
# the three rows: 4 x the worst of three runs on the MI355X (docs/kernels/counts.md), never looser than 1e-3
GRAD_MEASURED = 1.94e-10                                 # (1.94e-10 in each of the three: the variance is given, nothing is drawn)
GRAD_BAR = min(4 * GRAD_MEASURED, 1e-3)
DENSE_BAR = 10 * 1.43e-8                                 # test_gpu_nb.py: |device - dense float64| / logdet B


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


# ------------------------------------------------------------------------------------------------ 1: the kernel
def _inputs(n, seed):
    """f: half uniform in [-30, 12], half the special values up to +-1e4; counts from sizes on both sides of the digamma form's
    threshold up to 2^24; 70 % observed; float32 log-exposures of E in [0.5, 20]; var in [0.01, 9], u standard normal."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(-30.0, 12.0, n)
    f = np.where(rng.random(n) < 0.5, rng.choice(np.concatenate([SPECIAL, -SPECIAL]), n), f).astype(np.float32)
    y = rng.choice([0.0, 1.0, 2.0, 5.0, 31.0, 32.0, 33.0, 40.0, 1000.0, BIG], n).astype(np.float32)
    obs = rng.random(n) < 0.7
    obs[0] = True
    aux = np.log(rng.uniform(0.5, 20.0, n)).astype(np.float32)
    return f, y, aux, obs, rng.uniform(0.01, 9.0, n), rng.standard_normal(n)


def _nan(a, obs):
    return a if a is None or obs is None else np.where(obs, a, np.nan).astype(a.dtype)


def _up(dev, pad):
    """device copies, with pad one element off the vector boundary (a view into a larger buffer)"""
    if pad:
        return lambda a: None if a is None else T(np.concatenate([a[:1], a]), dev)[1:]
    return lambda a: None if a is None else T(a, dev)


def _check(dev, r, f, y, aux, obs, var, u, label, pad=False, h_floor=FLOOR):
    from manifold_gp_amd.counts import nb_dispersion_sums
    up = _up(dev, pad)
    args = (up(f), up(_nan(y, obs)), up(_nan(aux, obs)), up(obs), up(_nan(var, obs)), up(_nan(u, obs)))   # NaN at unobserved nodes
    if pad:
        assert args[0].data_ptr() % 16 == 4 and args[1].data_ptr() % 16 == 4 and (obs is None or args[3].data_ptr() % 4 == 1)
        assert (var is None or args[4].data_ptr() % 16 == 8) and (u is None or args[5].data_ptr() % 16 == 8)
    out = nb_dispersion_sums(*args, MEAN, r, h_floor)
    want, scale = dr.dispersion_sums(f, y, aux, obs, var, u, MEAN, r, h_floor)
    got = out.cpu().numpy()
    assert out.dtype == torch.float64 and out.shape == (3,) and np.isfinite(got).all()
    err = np.abs(got - want) / np.where(scale > 0, scale, 1.0)
    print("r = %g %s: rows within %.1e %.1e %.1e of their absolute terms (%.3g %.3g %.3g)" % (r, label, *err, *scale))
    assert (got[scale == 0] == 0).all() and err.max() <= ROW_BAR, (label, err)
    if var is None:
        assert got[1] == 0.0
    if u is None:
        assert got[2] == 0.0
    assert torch.equal(out, nb_dispersion_sums(*args, MEAN, r, h_floor))                      # bitwise: no atomics
    return out


@pytest.mark.parametrize("r", KERNEL_R)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_float64(dev, mgp, n, r):
    """mgp_nb_dispersion_sums against the float64 restatement on the same float32 inputs: every row within ROW_BAR of the sum of its
    absolute terms, |f| up to 1e4 and counts up to 2^24, NaN in y, aux, var and u at the unobserved 30 %, a second call bitwise
    equal.  n = 1: a lone node; 3: less than a quad; 4: one whole quad; 5: a quad and a tail; 257: past one workgroup's first
    sweep; 4099: several workgroups and a ragged tail.  Variants: var and u absent (rows 1 and 2 are 0 and the others unchanged),
    obs and aux NULL, every array one element off its 16-byte boundary -- bitwise the aligned call; the default floor."""
    f, y, aux, obs, var, u = _inputs(n, 7 * n + 1)
    full = _check(dev, r, f, y, aux, obs, var, u, "n = %d" % n)
    row0 = _check(dev, r, f, y, aux, obs, None, None, "n = %d, var and u NULL" % n)
    row01 = _check(dev, r, f, y, aux, obs, var, None, "n = %d, u NULL" % n)
    row02 = _check(dev, r, f, y, aux, obs, None, u, "n = %d, var NULL" % n)
    assert torch.equal(row0[0], full[0]) and torch.equal(row01[:2], full[:2]) and torch.equal(row02[2], full[2])
    _check(dev, r, f, y, None, None, var, u, "n = %d, obs and aux NULL" % n)
    shifted = _check(dev, r, f, y, aux, obs, var, u, "n = %d, one element off" % n, pad=True)
    assert torch.equal(shifted, full)
    _check(dev, r, f, y, aux, obs, var, u, "n = %d, default floor" % n, h_floor=eref.H_FLOOR)


def test_kernel_past_its_grid_cap(dev, mgp):
    """n = 1 051 653, beyond 1024 workgroups x 1024 nodes: the grid-stride loop runs twice in the first workgroups."""
    f, y, aux, obs, var, u = _inputs(CAP_N, 77)
    _check(dev, 1.5, f, y, aux, obs, var, u, "n = %d" % CAP_N)


def test_kernel_argument_errors(dev, mgp):
    """Every refusal comes before a launch: a NaN canary in out stays."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n = 64
    f = torch.zeros(n, device=dev)
    y = torch.ones(n, device=dev)
    var = torch.ones(n, dtype=torch.float64, device=dev)
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    work = torch.zeros(128, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()
    nan, inf = float("nan"), float("inf")

    def call(f_=f, y_=y, out_=out, n_=n, r=2.0, floor=1e-30, work_=work, wb=128, var_=var, u_=var):
        return lib.mgp_nb_dispersion_sums(p(f_), p(y_), None, None, p(var_), p(u_), n_, 0.0, r, floor, p(out_), p(work_), wb, st)
    assert call(f_=None) == -1 and call(y_=None) == -1 and call(out_=None) == -1 and call(n_=0) == -1 and call(n_=-1) == -1
    assert call(floor=-1.0) == -1 and call(floor=nan) == -1
    for r in (0.0, -1.0, 2.0 ** -11, 2.0 ** 20 + 1.0, nan, inf):
        assert call(r=r) == -1, r
    assert call(work_=None) == -2 and call(wb=31) == -2 and call(work_=work[4:]) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                                       # nothing was launched
    assert lib.mgp_nb_dispersion_sums_workspace_bytes(n) == 32 and call(wb=32) == 0
    assert call(var_=None, u_=None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and got[1] == 0.0 and got[2] == 0.0
    want, scale = dr.dispersion_sums(np.zeros(n), np.ones(n), None, None, None, None, 0.0, 2.0, 1e-30)
    assert abs(got[0] - want[0]) <= ROW_BAR * scale[0]


# ------------------------------------------------------------------------------------------------ 2: the gradient of a fit
_PROBLEM = {}


def _problem(mgp, golden, dev):
    """dumbbell_k10_loop, symmetric, nu = 2, built once: the descriptor scaled to the prior marginal variance
    _nb_ref.PRIOR_VARIANCE, the dense float64 matrix the kernels apply, the counts of _nb_ref.nb_counts on the device."""
    if not _PROBLEM:
        g = golden(CASE)
        d1 = _desc(mgp, g, dev, NORM, NU, scale=1.0)
        Q1 = oref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / nb.PRIOR_VARIANCE))
        c = nb.nb_counts(g)
        _PROBLEM.update(g=g, desc=d1.with_(scale=scale), Q=scale * Q1, scale=scale, counts=c, observed=T(c["obs"], dev), E=T(c["E"], dev),
                        y=T(np.where(c["obs"], c["y"], np.nan).astype(np.float32), dev))
    return _PROBLEM


def test_dispersion_gradient_of_a_fit(mgp, golden, dev):
    """r = 2, variance = the dense diag(A^-1) at the device's mode.  (a) dispersion_grad row by row against the float64
    dispersion_sums on the device's own mode, variance and u: 1e-12 of the absolute terms.  (b) its sum against the float64
    gradient at the float64 mode, relative to the sum of the absolute terms of the three rows: GRAD_BAR.  (c) backward() through a
    DispersionParameter gives r G for the raw parameter within 1e-12; no operator: neither probes nor X, Y.  (d) a dispersion that
    does not require grad, and none at all, take the same path: no solves, no gradient, and every part of the evidence that two
    calls of laplace_evidence(fit) reproduce is equal bit for bit -- the site sums, m, the log-likelihood, the quadratic part.
    logdet B is not such a part, with or without the new argument: a CG solve's iteration count depends on the solves that ran
    before it in the process (131, 137 and 138 iterations for three identical multi-column solves in a row, on a fresh plan cache
    too), so that three identical calls of laplace_evidence(fit) give logdet B = 0x1.8fae61ba16ea2p+6, 0x1.8fae61eecbb56p+6 and
    0x1.8fae61e3423e2p+6 (1e-9 relative; the same three in every process measured on the MI355X).  It is held to the dense bar of
    test_gpu_nb.py instead, 10 x 1.43e-8 of logdet B.  Measured: rows within 1.6e-18, 1.3e-16 and 0; the total 1.94e-10."""
    from manifold_gp_amd.counts import DispersionParameter, fit_counts
    from manifold_gp_amd.evidence import laplace_evidence
    p = _problem(mgp, golden, dev)
    r = 2.0
    d, Q = nb.data(p["counts"], r), p["Q"]
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
        fit = fit_counts(p["desc"], p["y"], p["observed"], family=NBF, dispersion=r, exposure=p["E"])
    assert fit.converged and fit.dispersion == r
    f = fit.mean.double().cpu().numpy()
    var = np.diag(np.linalg.inv(Q + np.diag(nb.curvature(f, d)))).copy()
    param = DispersionParameter(r)
    live = param()
    ev = laplace_evidence(fit, variance=T(var, dev), dispersion=live, solve_tol=1e-6)
    assert ev.dispersion_grad.shape == (3,) and ev.dispersion_grad.dtype == torch.float64 and ev.value.requires_grad
    assert set(ev.solves) == {"root_h", "corr", "w", "s_ref", "u"} and ev.solves["u"].dtype == torch.float64 and ev.cutpoint_grad is None
    rows, u = ev.dispersion_grad.cpu().numpy(), ev.solves["u"].cpu().numpy()
    want, scale = dr.dispersion_sums(f, d["y"], d["aux"], d["obs"], var, u, d["mean"], r)
    err = np.abs(rows - want) / scale
    print("dispersion_grad rows %s against float64 on the device's mode and u: %.1e %.1e %.1e of the absolute terms" % (rows, *err))
    assert err.max() <= 1e-12
    g64 = dr.dispersion_gradient(Q, d)
    G = float(rows.sum())
    rel = abs(G - g64["total"]) / g64["scale"].sum()
    print("d log Z / dr at r = 2: device %.9f, float64 at the float64 mode %.9f (rows %s): %.2e of the absolute terms %.4g; bar %.2e"
          % (G, g64["total"], g64["rows"], rel, g64["scale"].sum(), GRAD_BAR))
    assert rel <= GRAD_BAR
    ev.value.backward()
    got = float(param.raw.grad)
    assert param.raw.grad.dtype == torch.float64 and abs(got - r * G) <= 1e-12 * abs(r * G)
    plain = laplace_evidence(fit)
    fixed = laplace_evidence(fit, dispersion=live.detach())
    for e in (plain, fixed):
        assert e.dispersion_grad is None and e.solves is None and not e.value.requires_grad and e.method == "dense" and e.se == 0.0
    assert fixed.site_sums == plain.site_sums and fixed.m == plain.m                         # bitwise what it was
    assert fixed.log_likelihood == plain.log_likelihood and fixed.quad == plain.quad
    bar = DENSE_BAR * plain.logdet
    print("log Z without the argument %s, with a fixed dispersion %s, with its gradient %s; logdet B %s, %s"
          % (float(plain.value).hex(), float(fixed.value).hex(), float(ev.value.detach()).hex(), plain.logdet.hex(), fixed.logdet.hex()))
    assert abs(fixed.logdet - plain.logdet) <= bar and abs(float(fixed.value) - float(plain.value)) <= 0.5 * bar
    assert float(fixed.value) == plain.log_likelihood - plain.quad - 0.5 * fixed.logdet       # the same expression
    assert abs(float(ev.value.detach()) - float(plain.value)) <= 0.5 * bar                    # the surrogate adds exactly 0
    with pytest.raises(ValueError, match="not the fit's"):
        laplace_evidence(fit, dispersion=live.detach() * (1.0 + 2.0 ** -40))
    with pytest.raises(ValueError, match="0-dim float64"):
        laplace_evidence(fit, dispersion=2.0)


# ------------------------------------------------------------------------------------------------ 3: learning
def test_learn_dispersion_raises_the_dense_evidence(mgp, golden, dev):
    """From r = 16, 30 steps of Adam(0.1) with the kernel fixed: the dense float64 log Z at the returned dispersion exceeds the one
    at 16 by at least half the gain of the float64 run of the same optimiser (LEARN_GAIN = 43.05; test_nb_dispersion_cpu.py reruns
    it); the returned fit is an ordinary CountLaplaceFit."""
    from manifold_gp_amd.counts import CountLaplaceFit, learn_dispersion
    p = _problem(mgp, golden, dev)
    t, c, Q = dr.LEARN, p["counts"], p["Q"]
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*(learn_dispersion|laplace_fit).*")
        r, fit, history = learn_dispersion(p["desc"], p["y"], t["r0"], p["observed"], exposure=p["E"], steps=t["steps"], lr=t["lr"],
                                           var_samples=64)
    assert isinstance(fit, CountLaplaceFit) and fit.converged and fit.dispersion == r and len(history) == t["steps"]
    assert history[0][0] == t["r0"] and all(h[2] == 0.0 for h in history)                     # the dense path: no standard error
    z0 = nb.mode_log_z(Q, nb.data(c, t["r0"]))[1]["value"]
    z1 = nb.mode_log_z(Q, nb.data(c, r))[1]["value"]
    print("learn_dispersion: float64 run gains %.3f; device run r %.4g -> %.4f, dense log Z %.4f -> %.4f (gain %.3f); r by step %s"
          % (dr.LEARN_GAIN, t["r0"], r, z0, z1, z1 - z0, ["%.3f" % h[0] for h in history]))
    assert abs(history[0][1] - z0) <= 1e-5 * abs(z0)
    assert z1 - z0 >= 0.5 * dr.LEARN_GAIN
    lo, hi, reached = fit.predict_interval(0.9)                                                # an ordinary fit: predict_* works
    assert lo.shape == (p["desc"].n,) and bool(reached.all()) and bool((hi >= lo).all())


def test_laplace_train_raises_the_dense_evidence(mgp, golden, dev):
    """laplace_train(family="negative_binomial") for 10 epochs of Adam(0.1) on the raw length scale, the raw output scale and a
    DispersionParameter from r = 16 together, from _nb_dispersion_ref.TRAIN's start: the dense float64 log Z at the end exceeds the
    one at the start by at least half the gain of the float64 run (TRAIN_GAIN = 33.69; test_nb_dispersion_cpu.py reruns it); all
    three parameters moved.  Measured on the MI355X: a gain of 33.200 (length scale 0.7318, output scale 5.0787e-5, r = 6.18)."""
    from manifold_gp_amd.counts import DispersionParameter
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.utils import laplace_train
    t = dr.TRAIN
    g = golden(CASE)
    c = nb.nb_counts(g)
    x = T(g["train_x"], dev)
    y, obs, E = T(np.where(c["obs"], c["y"], np.nan).astype(np.float32), dev), T(c["obs"], dev), T(c["E"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=NU, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization=NORM, num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=t["kappa0"])
    model = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, t["scale0"]).to(dev)).to(dev)
    kern.raw_graphbandwidth.requires_grad_(False)
    param = DispersionParameter(t["r0"])
    opt = torch.optim.Adam([kern.raw_lengthscale, model.covar_module.raw_outputscale] + list(param.parameters()), lr=t["lr"])
    start = (float(kern.lengthscale), float(model.covar_module.outputscale), float(param().detach()))
    last = laplace_train(model, opt, observed=obs, family=NBF, max_iter=t["steps"] - 1, tolerance=0.0,
                         fit_kw=dict(dispersion=param, exposure=E), evidence_kw=dict(var_samples=64))
    end = (float(kern.lengthscale), float(model.covar_module.outputscale), float(param().detach()))

    def dense(kappa, scale, r):
        Q = eref.dense_q(g, NORM, NU, float(g["eps"]), kappa, scale).numpy()
        return nb.mode_log_z(0.5 * (Q + Q.T), nb.data(c, r))[1]["value"]
    z0, z1 = dense(*start), dense(*end)
    print("laplace_train: float64 run gains %.3f; device run %.4f -> %.4f (gain %.3f; kappa %.4f -> %.4f, scale %.5g -> %.5g, r %.4g -> "
          "%.4f), last loss %.5f" % (dr.TRAIN_GAIN, z0, z1, z1 - z0, start[0], end[0], start[1], end[1], start[2], end[2], last))
    assert start[2] == t["r0"] and np.isfinite(last) and all(a != b for a, b in zip(start, end))
    assert z1 - z0 >= 0.5 * dr.TRAIN_GAIN
    # a number keeps the fixed-dispersion path: the model method with a live dispersion agrees with it and adds the gradient
    fixed = model.laplace_evidence(observed=obs, family=NBF, dispersion=end[2], exposure=E, var_samples=64)
    livev = model.laplace_evidence(observed=obs, family=NBF, dispersion=param, exposure=E, var_samples=64)
    assert fixed.dispersion_grad is None and livev.dispersion_grad is not None
    assert float(fixed.value.detach()) == float(livev.value.detach())
