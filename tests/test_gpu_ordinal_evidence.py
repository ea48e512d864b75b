"""The evidence of the ordered-category fit on the MI355X (mgp_ordinal_evidence_site and mgp_ordinal_cut_sums in csrc/laplace.hip,
the ordinal family of manifold_gp_amd/evidence.py, CutpointParameter and learn_cutpoints of ordinal.py): the two kernels against
float64 on the same float32 inputs, the evidence, its cutpoint gradient and its hyper-parameter gradient against the dense float64
restatement (tests/_ordinal_evidence_ref.py), the two training loops against their float64 runs, and the model method."""
import warnings

import numpy as np
import pytest
import torch

import _evidence_ref as eref
import _observed_ref as obref
import _ordinal_evidence_ref as oev
import _ordinal_ref as oref
from test_gpu_evidence import DENSE_BAR, _rel_residual, check_theta
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

INF = np.inf
SITE_CAP_N = 1024 * 256 * 4 + 3 * 256 * 4 + 5          # beyond the grid cap of mgp_ordinal_evidence_site: 1024 workgroups x 1024 nodes
CUT_CAP_N = 1024 * 256 + 3 * 256 + 5                   # beyond the grid cap of mgp_ordinal_cut_sums: 1024 workgroups x 256 nodes
SIZES = [1, 3, 257, 4099]
CATEGORIES = [2, 3, 7, 64]
SPECIAL = np.array([0.0, 1e-8, 1.0, 20.0, 40.0, 88.0, 90.0, 200.0, 1e4])
FLOOR = 1e-6                                           # masks the nodes whose two ends both lie beyond 13.8 of f
K_FIT = 4
# The Lanczos comparison with the float64 quadrature on the same probes (frac = 0.5, 16 probes, 12 steps): 4 x the values measured
# on the MI355X (docs/kernels/evidence.md), never looser than 1e-3: value, |difference| / logdet B; standard error, |difference| / se
SLQ_MEASURED, SLQ_SE_MEASURED = 3.33e-7, 8.77e-7
SLQ_BAR, SLQ_SE_BAR = min(4 * SLQ_MEASURED, 1e-3), min(4 * SLQ_SE_MEASURED, 1e-3)
# the column sum of cutpoint_grad against the float64 gradient at the float64 mode, relative to the sum of the absolute terms of
# its column: 4 x the worst of the three cutpoints measured on the MI355X (docs/kernels/ordinal.md), never looser than 1e-3
CUT_MEASURED = 4.95e-9
CUT_BAR = min(4 * CUT_MEASURED, 1e-3)


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


# ------------------------------------------------------------------------------------------------ 1: the two kernels
def _cuts(K):
    """K - 1 cutpoints over [-3, 3.5], float32 values; from K = 3 on the second lies 2^-20 above the first"""
    b = (np.array([0.25]) if K == 2 else np.linspace(-3.0, 3.5, K - 1))
    if K >= 3:
        b[1] = b[0] + 2.0 ** -20
    return b.astype(np.float32).astype(np.float64)


def _inputs(n, K, seed):
    """f: half standard normal x 2, half the special values up to +-1e4; categories uniform over the K (infinite ends at 0 and
    K - 1, a gap of 2^-20 at category 1); 70 % observed; 2 % of the observed nodes carry a category >= K; var in [0.01, 9], u
    standard normal."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(n) * 2.0
    f = np.where(rng.random(n) < 0.5, rng.choice(np.concatenate([SPECIAL, -SPECIAL]), n), f).astype(np.float32)
    cat = rng.integers(0, K, n)
    lo, hi = oref.intervals(cat, _cuts(K))
    obs = rng.random(n) < 0.7
    obs[0] = True
    cat = np.where(rng.random(n) < 0.02, rng.integers(K, 255, n), cat).astype(np.uint8)
    return f, lo, hi, cat, obs, rng.uniform(0.01, 9.0, n), rng.standard_normal(n)


def _ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _up(dev, pad):
    return (lambda a: None if a is None else T(np.concatenate([a[:1], a]), dev)[1:]) if pad else (lambda a: None if a is None else T(a, dev))


def _nan(a, obs, fill=np.nan):
    return a if a is None or obs is None else np.where(obs, a, fill).astype(a.dtype)


def _check_site(dev, f, lo, hi, obs, var, label, pad=False, h_floor=FLOOR):
    from manifold_gp_amd.ordinal import ordinal_evidence_site
    up = _up(dev, pad)
    args = (up(f), up(_nan(lo, obs)), up(_nan(hi, obs)), up(obs), up(_nan(var, obs)))      # NaN wherever the node is unobserved
    if pad:
        assert args[0].data_ptr() % 16 == 4 and args[1].data_ptr() % 16 == 4 and (var is None or args[4].data_ptr() % 16 == 8)
    root, corr, sums = ordinal_evidence_site(*args, h_floor)
    want_root, want_corr, want_sums, scale, eff = oev.site_outputs(f, lo, hi, obs, var, h_floor)
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
    print("site %s: root_h %.2f ulp, corr %.2f ulp, sums %.1e %.1e %.1e, m = %d of %d observed, %d nodes"
          % (label, ur, uc, err[0], err[2], err[3], eff.sum(), len(f) if obs is None else obs.sum(), len(f)))
    assert err[0] <= 1e-12 and err[2] <= 1e-12 and err[3] <= 1e-14, (label, err)
    root2, corr2, sums2 = ordinal_evidence_site(*args, h_floor)
    assert torch.equal(root, root2) and torch.equal(sums, sums2) and (corr is None or torch.equal(corr, corr2))   # bitwise
    return (root, corr, sums), int(eff.sum()), int(len(f) if obs is None else obs.sum())


def _check_cuts(dev, f, lo, hi, cat, obs, var, u, K, label, pad=False, h_floor=FLOOR):
    from manifold_gp_amd.ordinal import ordinal_cut_sums
    up = _up(dev, pad)
    args = (up(f), up(_nan(lo, obs)), up(_nan(hi, obs)), up(_nan(cat, obs, 255)), up(obs), up(_nan(var, obs)), up(_nan(u, obs)))
    if pad:
        assert args[0].data_ptr() % 16 == 4 and args[3].data_ptr() % 4 == 1 and (var is None or args[5].data_ptr() % 16 == 8)
    out = ordinal_cut_sums(*args, K, h_floor)
    want, scale = oev.cut_sums(f, lo, hi, cat, obs, var, u, K, h_floor)
    got = out.cpu().numpy()
    assert out.dtype == torch.float64 and out.shape == (3, K - 1) and np.isfinite(got).all()
    assert (got[scale == 0] == 0).all()
    err = np.abs(got - want) / np.where(scale > 0, scale, 1.0)
    print("cut sums %s: rows within %.1e %.1e %.1e of their absolute terms (largest %.3g)" % (label, *err.max(1), scale.max()))
    assert err.max() <= 1e-12, (label, err.max(1))
    if var is None:
        assert not got[1].any()
    if u is None:
        assert not got[2].any()
    assert torch.equal(out, ordinal_cut_sums(*args, K, h_floor))                              # bitwise: no atomics
    return out


@pytest.mark.parametrize("K", CATEGORIES)
@pytest.mark.parametrize("n", SIZES)
def test_kernels_match_float64(dev, mgp, n, K):
    """mgp_ordinal_evidence_site: root_h and corr within 1 float32 ulp of the rounded float64 reference, 0 off the nodes kept, m
    exact, sum l and sum corr within 1e-12 of the sum of their absolute terms, max |corr| within 1e-14.  mgp_ordinal_cut_sums:
    every entry of the three rows within 1e-12 of the sum of its absolute terms.  |f| up to 1e4, a gap of 2^-20, infinite ends,
    30 % of the nodes unobserved with NaN in lo, hi, var, u and category 255, categories >= K at observed nodes; every node
    observed; var and u absent; second calls bitwise equal.  Measured on the MI355X: root_h and corr 0 ulp in every case, the site
    sums within 1.9e-16 (3.2e-16 past the grid cap), the rows within 3.8e-16 (1.2e-15 past it)."""
    f, lo, hi, cat, obs, var, u = _inputs(n, K, 1000 * K + n)
    label = "n = %d, K = %d" % (n, K)
    _, kept, seen = _check_site(dev, f, lo, hi, obs, var, label + ", 70 % observed")
    if n >= 257:
        assert 0 < kept < seen                                                                # the floor masks some, not all
    _check_site(dev, f, lo, hi, None, var, label + ", every node")
    _check_site(dev, f, lo, hi, obs, None, label + ", var NULL")
    full = _check_cuts(dev, f, lo, hi, cat, obs, var, u, K, label + ", 70 % observed")
    _check_cuts(dev, f, lo, hi, cat, None, var, u, K, label + ", every node")
    row0 = _check_cuts(dev, f, lo, hi, cat, obs, None, None, K, label + ", var and u NULL")
    row01 = _check_cuts(dev, f, lo, hi, cat, obs, var, None, K, label + ", u NULL")
    assert torch.equal(row0[0], full[0]) and torch.equal(row01[:2], full[:2])                 # the rows do not depend on each other


def test_kernels_past_their_grid_caps(dev, mgp):
    """One n beyond each kernel's grid cap: the grid-stride loop runs twice in the first workgroups."""
    f, lo, hi, cat, obs, var, u = _inputs(SITE_CAP_N, 7, 77)
    _check_site(dev, f, lo, hi, obs, var, "n = %d, K = 7" % SITE_CAP_N)
    n = CUT_CAP_N
    _check_cuts(dev, f[:n], lo[:n], hi[:n], cat[:n], obs[:n], var[:n], u[:n], 7, "n = %d, K = 7" % n)


@pytest.mark.parametrize("K", [2, 7])
def test_kernels_unaligned_arrays_and_the_default_floor(dev, mgp, K):
    """Arrays one element off a 16-byte boundary take the scalar path of the site kernel: the same bounds and the same outputs
    bit for bit as the aligned call, for both kernels.  Then the default floor H_FLOOR = 1e-30."""
    f, lo, hi, cat, obs, var, u = _inputs(257, K, 5)
    got, _, _ = _check_site(dev, f, lo, hi, obs, var, "n = 257, K = %d, one element off" % K, pad=True)
    want, _, _ = _check_site(dev, f, lo, hi, obs, var, "n = 257, K = %d, aligned" % K)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    a = _check_cuts(dev, f, lo, hi, cat, obs, var, u, K, "n = 257, K = %d, one element off" % K, pad=True)
    b = _check_cuts(dev, f, lo, hi, cat, obs, var, u, K, "n = 257, K = %d, aligned" % K)
    assert torch.equal(a, b)
    _, kept, seen = _check_site(dev, f, lo, hi, obs, var, "n = 257, default floor", h_floor=oev.H_FLOOR)
    assert kept < seen                                                                        # |f| = 1e4 stays masked
    _check_cuts(dev, f, lo, hi, cat, obs, var, u, K, "n = 257, default floor", h_floor=oev.H_FLOOR)
    # any integer type for the categories: the same sums as uint8
    from manifold_gp_amd.ordinal import ordinal_cut_sums
    args = [T(x, dev) for x in (f, lo, hi)]
    wide = ordinal_cut_sums(*args, T(cat.astype(np.int64), dev), T(obs, dev), T(var, dev), T(u, dev), K, FLOOR)
    assert torch.equal(wide, ordinal_cut_sums(*args, T(cat, dev), T(obs, dev), T(var, dev), T(u, dev), K, FLOOR))


def test_kernel_argument_errors(dev, mgp):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n, K = 64, 4
    f = torch.zeros(n, device=dev)
    hi = torch.ones(n, device=dev)
    cat = torch.zeros(n, dtype=torch.uint8, device=dev)
    var = torch.ones(n, dtype=torch.float64, device=dev)
    root, corr = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    sums = torch.zeros(4, dtype=torch.float64, device=dev)
    out = torch.full((3, K - 1), 7.0, dtype=torch.float64, device=dev)
    work = torch.zeros(128, dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def site(f_=f, lo_=f, hi_=hi, root_=root, sums_=sums, n_=n, floor=1e-30, work_=work, wb=128, corr_=corr):
        return lib.mgp_ordinal_evidence_site(p(f_), p(lo_), p(hi_), None, p(var), n_, floor, p(root_), p(corr_), p(sums_), p(work_), wb, st)
    assert site(f_=None) == -1 and site(lo_=None) == -1 and site(hi_=None) == -1 and site(root_=None) == -1 and site(sums_=None) == -1
    assert site(n_=0) == -1 and site(floor=-1.0) == -1 and site(floor=float("nan")) == -1 and site(work_=None) == -2 and site(wb=8) == -2
    torch.cuda.synchronize()
    assert bool((root == 7.0).all()) and bool((corr == 7.0).all()) and not sums.any()        # nothing was launched
    assert site(corr_=None) == 0
    torch.cuda.synchronize()
    assert bool((corr == 7.0).all()) and float(sums[2]) == 0.0 and float(sums[1]) == n        # corr NULL: not written
    assert site() == 0

    def cuts(f_=f, lo_=f, hi_=hi, cat_=cat, out_=out, n_=n, K_=K, floor=1e-30, work_=work, wb=128, var_=var, u_=var):
        return lib.mgp_ordinal_cut_sums(p(f_), p(lo_), p(hi_), p(cat_), None, p(var_), p(u_), n_, K_, floor, p(out_), p(work_), wb, st)
    assert cuts(f_=None) == -1 and cuts(lo_=None) == -1 and cuts(hi_=None) == -1 and cuts(cat_=None) == -1 and cuts(out_=None) == -1
    assert cuts(n_=0) == -1 and cuts(K_=1) == -1 and cuts(K_=65) == -1 and cuts(floor=-1.0) == -1 and cuts(floor=float("nan")) == -1
    assert cuts(work_=None) == -2 and cuts(wb=71) == -2 and cuts(K_=64, wb=128) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                           # nothing was launched
    assert cuts() == 0 and cuts(var_=None, u_=None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and not got[1:].any() and got[0, 0] > 0 and not got[0, 1:].any()   # every node in category 0


# ------------------------------------------------------------------------------------------------ 2: the evidence
_PROBLEMS = {}


def _problem(mgp, golden, dev, case, norm, nu, frac=0.1):
    """One ordinal problem per (fixture, normalisation, nu, frac), built once: the descriptor scaled to a prior marginal variance
    of about 9, the dense float64 matrix the kernels apply, the labels of _ordinal_ref.labels (K = 4), their frequency
    cutpoints, the device's fit and, at the device's mode, the float64 site values and the dense evidence."""
    key = (case, norm, nu, frac)
    if key not in _PROBLEMS:
        from manifold_gp_amd.ordinal import laplace_fit_ordinal
        g = golden(case)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = obref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        d = oev.data(g, K_FIT, frac)
        desc, Q = d1.with_(scale=scale), scale * Q1
        y, obs = T(np.where(d["obs"], d["y"], np.nan).astype(np.float32), dev), T(d["obs"], dev)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
            fit = laplace_fit_ordinal(desc, y, K_FIT, T(d["cuts"], dev), obs)
        assert fit.converged and np.array_equal(fit.cutpoints.cpu().numpy(), d["cuts"])
        f = fit.mean.double().cpu().numpy()
        lo, hi = oev.intervals64(d["y"], d["cuts"])
        l, _, h, hp = oev.site(f, lo, hi, d["obs"])
        eff = d["obs"] & (h >= oev.H_FLOOR)
        _PROBLEMS[key] = dict(g=g, desc=desc, Q=Q, scale=scale, d=d, y=y, obs=obs, fit=fit, f=f, lo=lo, hi=hi, l=l, h=h, hp=hp, eff=eff,
                              m=int(eff.sum()), z=oev.log_z(Q, f, d))
    return _PROBLEMS[key]


DENSE_CASES = [("dumbbell_k10_loop", "symmetric", 2), ("dumbbell_k10_loop", "randomwalk", 3), ("dumbbell_k50_noloop", "symmetric", 1)]


@pytest.mark.parametrize("case, norm, nu", DENSE_CASES)
def test_dense_logdet_and_the_evidence_value(mgp, golden, dev, case, norm, nu):
    """K = 4, 10 % observed: "auto" is the dense path; logdet B against the dense float64 value at the device's mode within the
    DENSE_BAR of test_gpu_evidence.py, the log-likelihood and the quadratic part within 1e-6 relative, the site kernel's sum of l
    plus sum log c_k equal to the fit's log-likelihood up to rounding.  The number differs from the Bernoulli evidence the call
    computed before it knew the ordinal fit (labels read as y > 0.5)."""
    from manifold_gp_amd.evidence import laplace_evidence
    p = _problem(mgp, golden, dev, case, norm, nu)
    z, fit, d = p["z"], p["fit"], p["d"]
    ev = fit.laplace_evidence()
    again = laplace_evidence(fit, method="dense")
    e_ld, e_ll, e_q = abs(ev.logdet - z["logdet"]) / z["logdet"], abs(ev.log_likelihood - z["log_likelihood"]) / abs(z["log_likelihood"]), \
        abs(ev.quad - z["quad"]) / z["quad"]
    print("%s %s nu = %d: m = %d, logdet B dense %.5f, device %.5f (relative %.2e); log Z %.5f, device %.5f; log-likelihood relative "
          "%.1e, quad relative %.1e" % (case, norm, nu, p["m"], z["logdet"], ev.logdet, e_ld, z["value"], float(ev.value), e_ll, e_q))
    assert p["m"] <= 512 and ev.method == "dense" and ev.m == p["m"] and ev.se == 0.0 and ev.per_probe is None
    assert e_ld <= DENSE_BAR and e_ll <= 1e-6 and e_q <= 1e-6
    assert ev.value.dtype == torch.float64 and ev.value.shape == () and not ev.value.requires_grad
    assert ev.solves is None and ev.cutpoint_grad is None
    # (the solver's tolerance split may adapt between two calls, so not bitwise)
    assert again.method == "dense" and abs(again.logdet - ev.logdet) <= 2 * DENSE_BAR * z["logdet"]
    const = float(oref.log_widths(d["cuts"])[d["y"]][d["obs"]].sum())
    l_abs = np.abs(p["l"]).sum()
    assert abs(ev.site_sums[0] + const - ev.log_likelihood) <= 2e-12 * l_abs + 4 * np.spacing(abs(ev.log_likelihood))
    assert ev.site_sums[1] == p["m"] and ev.site_sums[2] == 0.0 and ev.site_sums[3] == 0.0
    assert abs(float(ev.value) - z["value"]) <= 1e-6 * (abs(z["log_likelihood"]) + z["quad"]) + 0.5 * DENSE_BAR * z["logdet"]
    assert float(ev.value) == ev.log_likelihood - ev.quad - 0.5 * ev.logdet
    # what the call returned before: the Bernoulli curvature sigma'(f) at the labels read as y > 0.5
    _, h_b, _ = eref.site("bernoulli", p["f"], d["y"].astype(np.float64), None, d["obs"], 0.0)
    ld_b = eref.logdet_b(p["Q"], h_b, d["obs"] & (h_b >= eref.H_FLOOR))
    print("    the Bernoulli reading of the same fit: logdet B %.5f" % ld_b)
    assert abs(ev.logdet - ld_b) >= 1e-3 * z["logdet"] >= 1e3 * DENSE_BAR * z["logdet"]


def test_slq_matches_the_float64_quadrature_with_the_same_probes(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, half the nodes observed (m > 512: "auto" is Lanczos), 16 given probes and 12 steps against
    oracle.solvers.slq_logdet_same_probes on the dense B at the device's mode: value within SLQ_BAR of logdet B, the standard error
    within SLQ_SE_BAR relative, the estimate within 5 standard errors of the dense value."""
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2, frac=0.5)
    assert p["m"] > 512
    Z = eref.probes(p["eff"], eref.SLQ_PROBES, eref.SLQ_SEED)
    per_ref, want, se_ref = eref.slq_per_probe(eref.b_matmul(p["Q"], p["h"]), Z, eref.SLQ_STEPS, p["m"])
    ev = p["fit"].laplace_evidence(probes=T(Z.astype(np.float32), dev), steps=eref.SLQ_STEPS, solve_tol=1e-6)
    dense = p["z"]["logdet"]
    e_v, e_se = abs(ev.logdet - want) / dense, abs(ev.logdet_se - se_ref) / se_ref
    print("slq, m = %d: logdet B dense %.4f, device %.5f +- %.5f, float64 same probes %.5f +- %.5f: |difference| / logdet B = %.2e, se "
          "relative %.2e, worst probe %.2e of logdet B, %.2f standard errors from dense"
          % (p["m"], dense, ev.logdet, ev.logdet_se, want, se_ref, e_v, e_se, np.abs(ev.per_probe - per_ref).max() / dense,
             abs(ev.logdet - dense) / ev.logdet_se))
    assert ev.method == "slq" and ev.per_probe.shape == (eref.SLQ_PROBES,) and ev.se == 0.5 * ev.logdet_se
    assert e_v <= SLQ_BAR and e_se <= SLQ_SE_BAR
    assert abs(ev.logdet - dense) <= 5.0 * ev.logdet_se
    default = p["fit"].laplace_evidence(num_probes=eref.SLQ_PROBES, steps=eref.SLQ_STEPS, seed=eref.SLQ_SEED)
    assert abs(default.logdet - want) <= SLQ_BAR * dense                                      # the default probes are the restatement's


# ------------------------------------------------------------------------------------------------ 3: the gradients
def _dense_variance(p):
    return np.diag(np.linalg.inv(p["Q"] + np.diag(p["h"]))).copy()


def test_cutpoint_gradient(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, variance = the dense diag(A^-1) at the device's mode.  (a) cutpoint_grad row by row against
    the float64 cut_sums on the device's own mode and u: the kernel's bar, 1e-12 of the absolute terms.  (b) its column sum against
    the float64 gradient at the float64 mode of the same cutpoints, relative to the sum of the absolute terms: CUT_BAR.  (c)
    autograd through a CutpointParameter equals the chain rule of the column sum to 1e-12; no operator: neither probes nor X, Y."""
    from manifold_gp_amd.ordinal import CutpointParameter
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    d, fit, Q = p["d"], p["fit"], p["Q"]
    cut = CutpointParameter(K_FIT, torch.from_numpy(d["cuts"]))
    b = cut()
    assert np.array_equal(b.detach().float().double().numpy(), d["cuts"])
    var = _dense_variance(p)
    ev = fit.laplace_evidence(variance=T(var, dev), cutpoints=b, solve_tol=1e-6)
    rows = ev.cutpoint_grad.cpu().numpy()
    assert ev.cutpoint_grad.shape == (3, K_FIT - 1) and ev.cutpoint_grad.dtype == torch.float64 and ev.value.requires_grad
    assert set(ev.solves) == {"root_h", "corr", "w", "s_ref", "u"} and ev.solves["u"].dtype == torch.float64
    u = ev.solves["u"].cpu().numpy()
    want, scale = oev.cut_sums(p["f"], p["lo"], p["hi"], d["y"], d["obs"], var, u, K_FIT)
    err = np.abs(rows - want) / scale
    Adev = Q + np.diag(ev.solves["w"].double().cpu().numpy() / ev.solves["s_ref"])
    ru = _rel_residual(Adev, u[:, None], ev.solves["corr"].double().cpu().numpy()[:, None])
    print("cutpoint_grad rows against float64 on the device's mode and u: %.1e %.1e %.1e of the absolute terms; u true residual %.2e"
          % (*err.max(1), ru))
    assert err.max() <= 1e-12 and ru <= 2e-6
    f64 = oev.mode(Q, d)
    G64, rows64, scale64 = oev.cut_gradient(Q, f64, d)
    G = rows.sum(0)
    rel = np.abs(G - G64) / scale64.sum(0)
    print("d log Z / d b: device %s, float64 at the float64 mode %s: %s of the absolute terms %s"
          % (G, G64, ["%.2e" % v for v in rel], scale64.sum(0)))
    assert rel.max() <= CUT_BAR
    got, = torch.autograd.grad(ev.value, list(cut.parameters()))
    chain, = torch.autograd.grad((torch.from_numpy(G) * cut()).sum(), list(cut.parameters()))
    assert got.dtype == torch.float64 and float((got - chain).abs().max()) <= 1e-12 * float(chain.abs().max())
    plain = fit.laplace_evidence(cutpoints=b.detach())                                        # no grad asked for: the value alone
    assert plain.cutpoint_grad is None and plain.solves is None and not plain.value.requires_grad
    assert abs(float(plain.value) - float(ev.value.detach())) <= DENSE_BAR * p["z"]["logdet"]          # the surrogate adds exactly 0
    with pytest.raises(ValueError, match="fit.cutpoints"):
        fit.laplace_evidence(cutpoints=b + 1e-3)


def test_hyper_parameter_gradient_matches_float64_bilinear_forms(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, given probes and variance = the dense diag(A^-1): the gradients of the ordinal evidence with
    respect to graph bandwidth, length scale and output scale against the float64 derivatives of the three bilinear forms on the
    device's own u, X, Y and mode (oracle/grad_ref.py), within the operator-level bar of test_gpu_gradients.py (2e-4); the
    float64 true residuals of the three solves <= 2 tol; the cutpoints' gradient asked for in the same call shares u."""
    from oracle.grad_ref import bilinear_grads_f64
    from manifold_gp_amd.ordinal import CutpointParameter
    O = mgp.operators
    case, norm, nu, tol = "dumbbell_k10_loop", "symmetric", 2, 1e-6
    p = _problem(mgp, golden, dev, case, norm, nu)
    g, d, n, Q = p["g"], p["d"], p["desc"].n, p["Q"]
    theta = [float(np.float32(v)) for v in (float(g["eps"]), float(g["kappa"]), p["scale"])]
    th = [torch.tensor(v, device=dev, requires_grad=True) for v in theta]
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    lap = O.GraphLaplacianOperator(val, idx, n, th[0].view(1, 1), norm, bool(g["self_loops"]))
    op = O.ScaleWrapperOperator(O.PrecisionMaternOperator(lap, nu, th[1]), th[2])
    var = _dense_variance(p)
    P = eref.SLQ_PROBES
    Z = eref.probes(p["eff"], P, 4321)
    cut = CutpointParameter(K_FIT, torch.from_numpy(d["cuts"]))
    ev = p["fit"].laplace_evidence(operator=op, variance=T(var, dev), probes=T(Z.astype(np.float32), dev), solve_tol=tol, cutpoints=cut())
    assert ev.value.requires_grad and ev.method == "dense" and ev.cutpoint_grad is not None
    got = [float(x) for x in torch.autograd.grad(ev.value, th, retain_graph=True)]
    s = {k: (v.double().cpu().numpy() if torch.is_tensor(v) else v) for k, v in ev.solves.items()}
    f, u, X, Y = p["f"], s["u"], s["X"], s["Y"]
    V = np.concatenate([f[:, None], Y], 1)
    W = np.concatenate([0.5 * (u - f)[:, None], X * (0.5 / P)], 1)
    val64, idx64 = torch.from_numpy(g["edge_value"].astype(np.float64)), torch.from_numpy(g["edge_index"].astype(np.int64))
    ref, scale = bilinear_grads_f64(val64, idx64, n, theta + [0.0], nu, norm, bool(g["self_loops"]), V, W, stop="Q2")
    worst = check_theta(got, ref[:3], scale[:3], ["eps", "kappa", "outputscale"])
    SZ = s["root_h"][:, None] * s["Z"]
    Adev = Q + np.diag(s["w"] / s["s_ref"])
    rx, ry, ru = _rel_residual(Q, X, SZ), _rel_residual(Adev, Y, SZ), _rel_residual(Adev, u[:, None], s["corr"][:, None])
    exact = oev.gradient(Q, Q / p["scale"], f, d)[0]
    print("gradient (eps, kappa, outputscale) device %s, float64 on the device's vectors %s, worst %.4f of the bound; true residuals X "
          "%.2e, Y %.2e, u %.2e; output scale: dense analytic %.4f" % (["%.6f" % v for v in got], ["%.6f" % v for v in ref[:3]], worst,
                                                                      rx, ry, ru, exact))
    assert max(rx, ry, ru) <= 2.0 * tol
    assert ev.solves["X"].dtype == torch.float64 and ev.solves["u"].dtype == torch.float64 and ev.solves["Y"].dtype == torch.float32
    want, scale_c = oev.cut_sums(f, p["lo"], p["hi"], d["y"], d["obs"], var, u, K_FIT)
    assert (np.abs(ev.cutpoint_grad.cpu().numpy() - want) <= 1e-12 * scale_c).all()
    gc, = torch.autograd.grad(ev.value, list(cut.parameters()))
    assert bool(torch.isfinite(gc).all()) and float(gc.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 4: learning
def test_learn_cutpoints_raises_the_dense_evidence(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, K = 4, 10 % observed, from the frequency logits, 10 steps of Adam(0.1): the dense float64 log Z
    at the device run's cutpoints exceeds the one at the start by at least half the gain of learn_f64, the float64 run of the same
    optimiser with exact gradients (22.085; test_ordinal_evidence_cpu.py reruns it).  Measured on the MI355X: gains of 22.091,
    22.082 and 22.087 (the variance seed is drawn)."""
    from manifold_gp_amd.ordinal import OrdinalLaplaceFit, learn_cutpoints
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    t, d, Q = oev.LEARN, p["d"], p["Q"]
    gain64 = oev.LEARN_GAIN_F64
    assert gain64 >= 5.0
    cuts, fit, history = learn_cutpoints(p["desc"], p["y"], K_FIT, p["obs"], steps=t["steps"], lr=t["lr"], var_samples=64)
    assert isinstance(fit, OrdinalLaplaceFit) and fit.converged and len(history) == t["steps"]
    assert cuts.dtype == torch.float64 and torch.equal(cuts, fit.cutpoints) and cuts.data_ptr() != fit.cutpoints.data_ptr()
    end = dict(d, cuts=cuts.cpu().numpy())
    z0, z1 = p["z"]["value"], oev.log_z(Q, oev.mode(Q, end), end)["value"]
    print("learn_cutpoints: float64 run gains %.3f; device run %.4f -> %.4f (gain %.3f), cutpoints %s -> %s; log Z by step %s"
          % (gain64, z0, z1, z1 - z0, d["cuts"], end["cuts"], ["%.3f" % h[0] for h in history]))
    assert abs(history[0][0] - z0) <= 1e-5 * abs(z0) and all(h[1] == 0.0 for h in history)  # the dense path: no standard error
    assert z1 - z0 >= 0.5 * gain64
    proba, _ = fit.predict_proba(16, seed=3)                                                  # an ordinary fit: predict_* works
    assert proba.shape == (p["desc"].n, K_FIT) and float((proba.sum(1) - 1.0).abs().max()) <= 1e-9


def _model(mgp, g, dev, y, kappa, scale, norm="symmetric", nu=2, **kw):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    x = T(g["train_x"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization=norm, num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=kappa)
    return RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, scale).to(dev), **kw).to(dev), kern


def test_laplace_train_raises_the_dense_evidence(mgp, golden, dev):
    """laplace_train(family="ordinal") for 10 epochs of Adam(0.1) on the raw length scale, the raw output scale and a
    CutpointParameter together, from _evidence_ref.TRAIN's start and the frequency logits: the dense float64 log Z at the end
    exceeds the one at the start by at least half the gain of train_f64 (22.457; test_ordinal_evidence_cpu.py reruns it).
    Measured on the MI355X: gains of 22.402, 22.381 and 22.354."""
    from manifold_gp_amd.ordinal import CutpointParameter
    from manifold_gp_amd.utils import laplace_train
    t = eref.TRAIN
    case, norm, nu = "dumbbell_k10_loop", "symmetric", 2
    g = golden(case)
    d = oev.data(g, K_FIT, oev.LEARN["frac"])
    gain64 = oev.TRAIN_GAIN_F64
    assert gain64 >= 5.0
    y, obs = T(np.where(d["obs"], d["y"], np.nan).astype(np.float32), dev), T(d["obs"], dev)
    model, kern = _model(mgp, g, dev, y, t["kappa0"], t["scale0"])
    kern.raw_graphbandwidth.requires_grad_(False)
    cut = CutpointParameter(K_FIT, torch.from_numpy(d["cuts"]))
    opt = torch.optim.Adam([kern.raw_lengthscale, model.covar_module.raw_outputscale] + list(cut.parameters()), lr=t["lr"])
    start = (float(kern.lengthscale), float(model.covar_module.outputscale), cut().detach().numpy().copy())
    last = laplace_train(model, opt, observed=obs, family="ordinal", max_iter=t["steps"] - 1, tolerance=0.0,
                         fit_kw=dict(num_categories=K_FIT, cutpoints=cut), evidence_kw=dict(var_samples=64))
    end = (float(kern.lengthscale), float(model.covar_module.outputscale), cut().detach().numpy().copy())

    def dense(kappa, scale, cuts):
        Q = eref.dense_q(g, norm, nu, float(g["eps"]), kappa, scale).numpy()
        dk = dict(d, cuts=cuts)
        return oev.log_z(Q, oev.mode(Q, dk), dk)["value"]
    z0, z1 = dense(*start), dense(*end)
    print("laplace_train: float64 run gains %.3f; device run %.4f -> %.4f (gain %.3f; kappa %.4f -> %.4f, scale %.5g -> %.5g, cutpoints "
          "%s -> %s), last loss %.5f" % (gain64, z0, z1, z1 - z0, start[0], end[0], start[1], end[1], start[2], end[2], last))
    assert np.isfinite(last) and not np.array_equal(start[2], end[2]) and start[0] != end[0] and start[1] != end[1]
    assert z1 - z0 >= 0.5 * gain64


# ------------------------------------------------------------------------------------------------ 5: the model method
def test_model_method_agrees_with_the_fit(mgp, golden, dev):
    from manifold_gp_amd.evidence import LaplaceEvidence
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.ordinal import CutpointParameter, ordinal_cutpoints
    g = golden("dumbbell_k10_loop")
    d = oev.data(g, K_FIT, 0.1)
    y, obs = T(np.where(d["obs"], d["y"], np.nan).astype(np.float32), dev), T(d["obs"], dev)
    model, kern = _model(mgp, g, dev, y, float(g["kappa"]), 1.1e-5)
    # a CutpointParameter: the fit at its detached values, the live tensor to the evidence.  (First, as in test_gpu_evidence.py:
    # the solver's tolerance split may adapt during the first solves of a shape, and the two calls compared bit for bit below
    # come after it.)
    cut = CutpointParameter(K_FIT, ordinal_cutpoints(y, K_FIT, obs))
    c = model.laplace_evidence(observed=obs, family="ordinal", num_categories=K_FIT, cutpoints=cut, method="slq", seed=11, rtol=1e-5)
    assert c.value.requires_grad and c.cutpoint_grad is not None and c.solves is not None and "X" in c.solves
    grads = torch.autograd.grad(c.value, [kern.raw_lengthscale] + list(cut.parameters()))
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in grads)
    with torch.no_grad():
        a = model.laplace_evidence(observed=obs, family="ordinal", num_categories=K_FIT, method="slq", seed=11, rtol=1e-5)
        fit = model.laplace_posterior_ordinal(K_FIT, observed=obs, rtol=1e-5)
        b = fit.laplace_evidence(method="slq", seed=11)
        assert isinstance(a, LaplaceEvidence) and a.method == "slq" and a.se > 0.0 and not a.value.requires_grad
        assert torch.equal(a.value, b.value) and a.logdet == b.logdet and a.se == b.se and np.array_equal(a.per_probe, b.per_probe)
        # fit_kw / evidence_kw name the receiver; the cutpoints go to the fit
        e = model.laplace_evidence(observed=obs, family="ordinal", max_iter=4000, fit_kw=dict(num_categories=K_FIT, rtol=1e-5, cutpoints=fit.cutpoints),
                                   evidence_kw=dict(method="slq", seed=11, max_iter=3000))
        assert abs(float(e.value) - float(a.value)) <= 1e-6 * abs(float(a.value))
        with pytest.raises(TypeError):
            model.laplace_evidence(observed=obs, family="ordinal", num_categories=K_FIT, evidence_kw=dict(rtol=1e-5))
        with pytest.raises(ValueError, match="num_categories"):
            model.laplace_evidence(observed=obs, family="ordinal")
    assert abs(float(c.value.detach()) - float(a.value)) <= 1e-3 * abs(float(a.value))       # the surrogates add exactly 0
    assert torch.equal(fit.cutpoints.cpu(), cut().detach().float().double())
    with pytest.raises(ValueError, match="family"):
        model.laplace_evidence(observed=obs, family="probit")
    semi = RiemannGP(model.train_inputs[0], y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev),
                     labeled=T(np.arange(y.shape[0]) < 100, dev)).to(dev)
    with pytest.raises(NotImplementedError):
        semi.laplace_evidence(observed=obs, family="ordinal", num_categories=K_FIT)
