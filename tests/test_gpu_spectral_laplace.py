"""Laplace fits on the spectral features on the MI355X (csrc/spectral_laplace.hip, manifold_gp_amd/spectral_laplace.py): the
entry point against its float64 restatement on the same float32 Z, the fit on the dumbbell fixtures against the dense float64
Newton iteration, the latent values and every predictive output at test points, the evidence against the dense function-space
formula, and the model method (tests/_spectral_laplace_ref.py)."""
import warnings

import numpy as np
import pytest
import torch

import _spectral_laplace_ref as sref

pytestmark = pytest.mark.gpu

FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]
# the kernels' own caps (csrc/spectral_laplace.hip): kSpecMaxBlocks workgroups x 4 rows per step of the site kernel;
# kGramMaxChunks row chunks x kGramMinRows rows of the Gram kernel before a chunk grows
SITE_GRID_CAP, SITE_ROWS_PER_STEP = 512, 4
GRAM_MAX_CHUNKS, GRAM_MIN_ROWS = 128, 128
N_PAST = max(SITE_GRID_CAP * SITE_ROWS_PER_STEP, GRAM_MAX_CHUNKS * GRAM_MIN_ROWS) + 33
SHAPES = ([(n, 100) for n in (1, 31, 32, 33, 64, 257, 1546)] + [(257, m) for m in (1, 3, 4, 63, 64, 65, 128, 130, 512)]
          + [(N_PAST, 100)])
MASKS = ["tenth", "all", "stages"]
BAR = 1e-12               # of the sum of the absolute terms: the bar of the site sums in test_gpu_laplace.py
RULE_ERROR = 1.08e-9      # relative error of the count pmf's quadrature at its default points, v <= 9 (docs/kernels/count_predict.md)
SUM_ROUNDING = 2.0 ** -45 # a float64 sum of up to 1025 quadrature terms no larger than 1


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


def T(a, dev, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------ 1: the entry point
def _mask(kind, n, rng):
    if kind == "all":
        return np.ones(n, bool)
    if kind == "tenth":
        obs = rng.random(n) < 0.1
    else:                                                  # two of three 32-row stages hold no observed row
        obs = (rng.random(n) < 0.5) & ((np.arange(n) // 32) % 3 == 0)
    obs[0] = True
    return obs


def _kernel_case(family, n, m, kind, seed):
    rng = np.random.default_rng(seed)
    Z = sref.f32(rng.standard_normal((n, m)) / np.sqrt(m))
    w = 1.5 * rng.standard_normal(m)
    obs = _mask(kind, n, rng)
    d, _ = sref.problem(family, 0.7 * (Z @ w), obs, seed + 1, mean=0.25)
    return Z, w, d


def _call(dev, Z, w, d, hessian=True, nan_outside=False, all_rows=False, Zt=None):
    from manifold_gp_amd.spectral_laplace import spectral_site
    a, b, obs = d["a"], d["b"], d["obs"]
    if nan_outside:
        a = np.where(obs, a, np.nan)
        b = None if b is None else np.where(obs, b, np.nan)
    Zt = T(Z, dev, torch.float32) if Zt is None else Zt
    out = spectral_site(Zt, T(w, dev), d["family"], T(a, dev, torch.float32), None if b is None else T(b, dev, torch.float32),
                        None if all_rows else T(obs, dev), d["mean"], d["r"], hessian)
    return out


def _np(t):
    return t.cpu().numpy()


def _errors(got, Z, w, d):
    """the four outputs against the restatement, each error as a multiple of the sum of its absolute terms"""
    f, grad, hess, sums = (_np(t) for t in got)
    rf, rgrad, rhess, rsums, scale = sref.site_outputs(Z, w, d)
    assert np.isfinite(f).all() and np.isfinite(grad).all() and np.isfinite(hess).all() and np.isfinite(sums).all()

    def rel(x, y, s):
        err = np.abs(x - y)
        assert (err[s == 0] == 0).all()
        return float((err[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0
    assert sums[1] == np.abs(f).max()                      # the maximum of the kernel's own f: exact
    return (rel(f, rf, scale["f"]), rel(grad, rgrad, scale["grad"]), rel(hess, rhess, scale["hess"]),
            rel(sums[:1], rsums[:1], np.array([scale["lp"]])))


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("family", sref.FAMILIES)
def test_site_matches_float64(mgp, dev, family, n, m):
    """f, grad, hess and sums[0] within 1e-12 of the sum of their absolute terms, sums[1] exact; hess bitwise symmetric; a second
    call and the call without a Hessian bitwise equal; 10 % observed, every row, and whole 32-row stages unobserved."""
    for kind in MASKS:
        Z, w, d = _kernel_case(family, n, m, kind, 100 * n + m)
        got = _call(dev, Z, w, d, all_rows=kind == "all")
        errs = _errors(got, Z, w, d)
        print("%s n=%d m=%d %s: f %.1e grad %.1e hess %.1e lp %.1e" % (family, n, m, kind, *errs))
        assert max(errs) <= BAR, (family, n, m, kind, errs)
        f, grad, hess, sums = got
        assert hess.dtype == torch.float64 and hess.shape == (m, m) and torch.equal(hess, hess.T.contiguous())
        again = _call(dev, Z, w, d, all_rows=kind == "all")
        assert all(torch.equal(x, y) for x, y in zip(got, again))
        f2, grad2, none, sums2 = _call(dev, Z, w, d, hessian=False, all_rows=kind == "all")
        assert none is None and torch.equal(f, f2) and torch.equal(grad, grad2) and torch.equal(sums, sums2)


@pytest.mark.parametrize("family", sref.FAMILIES)
@pytest.mark.parametrize("n,m", [(257, 100), (257, 65), (33, 512)])
def test_site_unaligned_view_and_nan_outside(mgp, dev, family, n, m):
    """A Z view one float off 16-byte alignment gives the same numbers within the bar; NaN in a and b at unobserved rows changes
    no bit."""
    Z, w, d = _kernel_case(family, n, m, "tenth", 7 * n + m)
    base = _call(dev, Z, w, d)
    buf = torch.zeros(n * m + 1, dtype=torch.float32, device=dev)
    buf[1:] = T(Z, dev, torch.float32).reshape(-1)
    view = buf[1:].view(n, m)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    off = _call(dev, Z, w, d, Zt=view)
    errs = _errors(off, Z, w, d)
    print("%s n=%d m=%d off alignment: f %.1e grad %.1e hess %.1e lp %.1e" % (family, n, m, *errs))
    assert max(errs) <= BAR
    assert torch.equal(off[2], off[2].T.contiguous())
    nan = _call(dev, Z, w, d, nan_outside=True)
    assert all(torch.equal(x, y) for x, y in zip(base, nan))


@pytest.mark.parametrize("family", sref.FAMILIES)
def test_site_finite_at_large_latent_values(mgp, dev, family):
    """w scaled so that max |f| = 1e4: every output finite (the Poisson exp is clamped at 700)"""
    Z, w, d = _kernel_case(family, 257, 100, "all", 11)
    w = w * (1e4 / np.abs(Z @ w).max())
    f, grad, hess, sums = (_np(t) for t in _call(dev, Z, w, d))
    assert abs(sums[1] - 1e4) <= 1e-8
    for t in (f, grad, hess, sums):
        assert np.isfinite(t).all()


def test_site_entry_point_refuses_before_launching(mgp, dev):
    """the C entry point's own checks (csrc/spectral_laplace.hip): null pointers, m > 512, a missing b, a short workspace"""
    from manifold_gp_amd._lib import lib, ptr, stream
    n, m = 64, 8
    Z = torch.zeros(n, m, device=dev)
    w = torch.zeros(m, dtype=torch.float64, device=dev)
    a = torch.zeros(n, device=dev)
    grad = torch.full((m,), 7.0, dtype=torch.float64, device=dev)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    nbytes = lib().mgp_spectral_site_workspace_bytes(n, m, 0)
    assert nbytes > 0 and lib().mgp_spectral_site_workspace_bytes(n, 513, 1) == 0
    assert lib().mgp_spectral_site_workspace_bytes(n, m, 1) > nbytes
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(Z=Z, m=m, fam=0, a=a, b=None, r=0.0, grad=grad, nbytes=nbytes):
        return lib().mgp_spectral_site(ptr(Z), n, m, ptr(w), fam, ptr(a), ptr(b), None, 0.0, r, None, ptr(grad), None, ptr(sums),
                                       ptr(work), nbytes, stream())
    assert call() == 0
    torch.cuda.synchronize()
    grad.fill_(7.0)
    sums.fill_(7.0)
    ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3
    for code in (call(Z=None), call(a=None), call(grad=None), call(m=513), call(m=0), call(fam=2), call(fam=4), call(fam=3, r=0.0),
                 call(fam=3, r=float("nan"))):
        assert code == ERR_ARG
    assert call(fam=5) == ERR_UNSUPPORTED and call(fam=-1) == ERR_UNSUPPORTED
    assert call(nbytes=nbytes - 1) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and bool((sums == 7.0).all())          # nothing was launched


# ------------------------------------------------------------------------------------------------ 2 - 4: the fit
_MODELS = {}


def _model(mgp, golden, dev, case):
    """The fixture's model after eval(), built once: 50 modes (the golden's), random-walk Laplacian, nu = 2, the outputscale set to
    a prior marginal variance of about 9 at the training rows (|f_hat| of a few units: the likelihoods are far from linear)."""
    if case not in _MODELS:
        from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
        g = golden(case)
        x = T(g["train_x"], dev)
        kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                               num_modes=int(g["modes"]), bump_scale=float(g["bump"][0]),
                                               bump_decay=float(g["bump"][1])).to(dev)
        kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
        y = torch.zeros(x.shape[0], device=dev)
        model = RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
        model.eval()
        with torch.no_grad():
            Z = kern.features(x)
            Zs = kern.features(T(g["test_x"], dev))
        s = float(np.float32(9.0 / float((Z.double() ** 2).sum(1).mean())))
        model.covar_module.outputscale = s
        s = float(model.covar_module.outputscale.detach())  # what the model hands to the fit
        _MODELS[case] = dict(g=g, model=model, kern=kern, Z=Z, Zs=Zs, s=s, Z64=_np(Z).astype(np.float64),
                             Zs64=_np(Zs).astype(np.float64), fits={})
    return _MODELS[case]


def _fit_case(mgp, golden, dev, case, family):
    """One fit per (fixture, family), shared by the tests below: data simulated with a seed from 1.2 x the standardised first
    coordinate (the latent function of the node fits' tests), 10 % of the rows observed; the fit, the float64 Newton restatement
    on the same Z, and the bound of their distance from both final gradients."""
    M = _model(mgp, golden, dev, case)
    if family not in M["fits"]:
        from manifold_gp_amd.spectral_laplace import spectral_laplace_fit
        x0 = M["g"]["train_x"][:, 0].astype(np.float64)
        ftrue = 1.2 * (x0 - x0.mean()) / x0.std()
        rng = np.random.default_rng(17)
        obs = rng.random(x0.shape[0]) < 0.10
        mean = 1.0 if family in ("poisson", "negative_binomial") else 0.0
        d, pub = sref.problem(family, ftrue, obs, 23, mean=mean)
        kw = {k: (v if np.isscalar(v) else T(v, dev, torch.float64)) for k, v in pub.items() if v is not None and k != "y"}
        if "num_categories" in kw:
            kw["num_categories"] = int(kw["num_categories"])
        y = np.where(obs, pub["y"], np.nan)                # nothing outside `observed` is read
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*spectral_laplace_fit.*")
            fit = spectral_laplace_fit(M["Z"], T(y, dev, torch.float64), T(obs, dev), family, outputscale=M["s"], mean=mean, **kw)
        Z, s = M["Z64"], M["s"]
        w_ref, g_ref, trace = sref.newton(Z, d, s, rtol=1e-12)
        w_fit = _np(fit.weights)
        g_fit = sref.gradient(Z, d, s, w_fit)
        bound = sref.weight_bound(s, [g_fit, g_ref], [sref.gradient_rounding(Z, d, s, w_ref)] * 2)
        M["fits"][family] = dict(d=d, pub=pub, fit=fit, w_ref=w_ref, w_fit=w_fit, bound=bound, steps=len(trace), mean=mean)
    return M, M["fits"][family]


def _input_bounds(M, c, Zs):
    """(d_eta, d_var) per test row: how far the fit's (eta, var) may lie from the restatement's.  |d eta| <= |z*| |dw|.
    var = z*^T A^-1 z* with |A^-1| <= s: |d var| <= s^2 |z*|^2 |dA|, |dA| <= sum_i |z_i|^2 |dh_i|, |dh_i| <= L_i |z_i| |dw| with L_i
    the bound of |h'| (doubled: it is taken at the restatement's mode, the fit's lies within |dw| of it); on top the rounding
    of the m x m Cholesky solve, 4 m 2^-52 cond(A) of s |z*|^2."""
    Z, s, d, dw = M["Z64"], M["s"], c["d"], c["bound"]
    zn = np.linalg.norm(Zs, axis=1)
    rn = np.linalg.norm(Z, axis=1)
    dA = float((rn ** 3 * 2.0 * sref.h_prime_bound(d, Z @ c["w_ref"])).sum()) * dw
    A = sref.hessian(Z, d, s, c["w_ref"])
    solve = 4.0 * A.shape[0] * sref.EPS * np.linalg.cond(A) * s * zn ** 2
    return zn * dw + sref.EPS * (np.abs(Zs) @ np.abs(c["w_ref"]) + abs(c["mean"])), s * s * zn ** 2 * dA + solve


@pytest.mark.parametrize("family", sref.FAMILIES)
@pytest.mark.parametrize("case", FIXTURES)
def test_fit_matches_dense_float64_newton(mgp, golden, dev, case, family):
    """The weights within s (|grad psi(w_fit)| + |grad psi(w_ref)|) of the float64 restatement's (A >= I / s), the bound computed
    here from both final gradients; converged without a warning; the training rows' latent values are Z w + mean."""
    M, c = _fit_case(mgp, golden, dev, case, family)
    fit = c["fit"]
    diff = float(np.linalg.norm(c["w_fit"] - c["w_ref"]))
    print("%s %s: %d steps (float64: %d), relative gradient %.1e, |dw| %.2e, bound %.2e, max |f| %.2f"
          % (case, family, fit.iterations, c["steps"], fit.history[-1][1], diff, c["bound"], float(fit.mean.abs().max())))
    assert fit.converged and fit.history[-1][1] <= 1e-10
    assert fit.weights.dtype == torch.float64 and fit.chol.shape == (M["Z"].shape[1],) * 2
    assert diff <= c["bound"]
    want = M["Z64"] @ c["w_fit"] + c["mean"]
    assert np.abs(_np(fit.mean) - want).max() <= BAR * (np.abs(M["Z64"]) @ np.abs(c["w_fit"]) + abs(c["mean"])).max()
    assert all(b[0] >= a[0] - 2.0 ** -40 * abs(a[0]) for a, b in zip(fit.history, fit.history[1:]))       # psi never decreases


@pytest.mark.parametrize("family", sref.FAMILIES)
@pytest.mark.parametrize("case", FIXTURES)
def test_latent_and_predictions_at_test_points(mgp, golden, dev, case, family):
    """latent(features(test_x)) against numpy on the same Z* and weights; every predictive output against the same predictive
    function on the restatement's (eta, var), within the input difference (_input_bounds) times the function's Lipschitz
    constant; predicted classes identical except where the restatement's probability lies within that bar of the boundary."""
    from manifold_gp_amd.classification import bernoulli_predict
    from manifold_gp_amd.counts import count_predict_logpmf, count_predict_pmf
    from manifold_gp_amd.ordinal import ordinal_predict
    M, c = _fit_case(mgp, golden, dev, case, family)
    fit, d, s = c["fit"], c["d"], M["s"]
    Zs, Zs64 = M["Zs"], M["Zs64"]
    Tn = Zs64.shape[0]
    eta, var = fit.latent(Zs)
    # (a) numpy on the same Z* with the fit's own weights
    eta_np, var_np = sref.latent(Zs64, d, s, M["Z64"], c["w_fit"])
    A = sref.hessian(M["Z64"], d, s, c["w_fit"])
    zn2 = (Zs64 ** 2).sum(1)
    e_eta = np.abs(_np(eta) - eta_np) / (np.abs(Zs64) @ np.abs(c["w_fit"]) + abs(c["mean"]))
    var_bar = 4.0 * A.shape[0] * sref.EPS * np.linalg.cond(A) * s * zn2 * 2.0          # the two solves' rounding
    print("%s %s: eta %.1e of its terms, var within %.1e of its bar" % (case, family, e_eta.max(), (np.abs(_np(var) - var_np) / var_bar).max()))
    assert e_eta.max() <= BAR and (np.abs(_np(var) - var_np) <= var_bar).all() and (_np(var) >= 0).all()
    # (b) the predictive functions on the restatement's (eta, var)
    eta_r, var_r = sref.latent(Zs64, d, s, M["Z64"], c["w_ref"])
    d_eta, d_var = _input_bounds(M, c, Zs64)
    assert (np.abs(_np(eta) - eta_r) <= d_eta).all() and (np.abs(_np(var) - var_r) <= d_var).all()
    te, tv = T(eta_r, dev), T(var_r, dev)
    quarter, tenth = 0.25, 0.1                             # max sigma' and an upper bound of max |sigma''| (1 / (6 sqrt 3)), doubled for
                                                           # the two sigmoids of an ordinal category: the second of E sigma(eta + sqrt(v) u)
                                                           # in v is E sigma'' / 2
    if family == "bernoulli":
        p, pr = _np(fit.predict_proba(Zs)), _np(bernoulli_predict(te, tv))
        bar = quarter * (d_eta + np.spacing(np.abs(eta_r).astype(np.float32)).astype(np.float64)) + tenth * d_var + SUM_ROUNDING
        assert (np.abs(p - pr) <= bar).all()
        excused = np.abs(pr - 0.5) <= bar
        assert ((p > 0.5) == (pr > 0.5))[~excused].all() and excused.sum() <= 0.01 * Tn
        yt = (np.arange(Tn) % 2).astype(np.float64)
        ld = _np(fit.predict_log_density(Zs, T(yt, dev)))
        want = np.where(yt > 0.5, np.log(pr), np.log1p(-pr))
        assert (np.abs(ld - want) <= bar / np.minimum(pr, 1.0 - pr) + 4 * sref.EPS).all()
    elif family == "ordinal":
        cuts = T(c["pub"]["cutpoints"], dev, torch.float64)
        p, pr = _np(fit.predict_proba(Zs)), _np(ordinal_predict(te, tv, cuts))
        bar = (quarter * d_eta + 2.0 * tenth * d_var + SUM_ROUNDING)[:, None]
        assert p.shape == (Tn, 4) and (np.abs(p - pr) <= bar).all() and np.abs(p.sum(1) - 1.0).max() <= 1e-12
        top = np.sort(pr, axis=1)
        excused = top[:, -1] - top[:, -2] <= 2.0 * bar[:, 0]
        assert (p.argmax(1) == pr.argmax(1))[~excused].all() and excused.sum() <= 0.01 * Tn
        yt = np.arange(Tn) % 4
        ld = _np(fit.predict_log_density(Zs, T(yt, dev)))
        want = np.log(pr[np.arange(Tn), yt])
        assert (np.abs(ld - want) <= bar[:, 0] / pr[np.arange(Tn), yt] + 64 * sref.EPS).all()
    else:
        rng = np.random.default_rng(3)
        kmax = 24
        if family == "binomial":
            N = rng.integers(1, 40, Tn).astype(np.float64)
            aux_kw, aux_r, eta_in = dict(trials=T(N, dev, torch.float64)), T(N, dev, torch.float32), eta_r
            L1 = N
            L2 = 0.5 * (N ** 2 + N / 4.0)
        else:
            E = rng.uniform(0.5, 20.0, Tn)
            aux_kw, aux_r, eta_in = dict(exposure=T(E, dev, torch.float64)), None, eta_r + np.log(E)
            if family == "poisson":                        # |p'| <= p |k - mu|, |p''| <= p ((k - mu)^2 + mu), mu up to exp(eta + 2 v)
                mu_hi = np.exp(eta_in + 2.0 * var_r)
                L1 = kmax + mu_hi
                L2 = 0.5 * (L1 ** 2 + mu_hi)
            else:                                          # |g| <= k + r, h <= (k + r) / 4
                L1 = np.full(Tn, kmax + d["r"])
                L2 = 0.5 * (L1 ** 2 + L1 / 4.0)
        tin = T(eta_in, dev)
        lip = L1 * d_eta + L2 * d_var
        pmf = _np(fit.predict_pmf(Zs, kmax, **aux_kw))
        pmf_r = _np(count_predict_pmf(tin, tv, aux_r, family, 0, kmax, dispersion=d["r"]))
        assert pmf.shape == (Tn, kmax + 1)
        assert (np.abs(pmf - pmf_r) <= lip[:, None] + 2.0 * RULE_ERROR * pmf_r + 1e-300).all()
        yt = np.minimum(rng.integers(0, kmax, Tn).astype(np.float64), N if family == "binomial" else kmax)
        ld = _np(fit.predict_log_density(Zs, T(yt, dev, torch.float64), **aux_kw))
        ld_r = _np(count_predict_logpmf(tin, tv, aux_r, T(yt, dev, torch.float32), None, family, dispersion=d["r"]))
        assert (np.abs(ld - ld_r) <= lip / np.exp(ld_r) + 2.0 * RULE_ERROR).all()
        mean, pvar = (_np(t) for t in fit.predict_mean(Zs, **aux_kw))
        if family == "binomial":
            from manifold_gp_amd.classification import bernoulli_predict as bp
            pr = _np(bp(te, tv))
            bar = quarter * (d_eta + np.spacing(np.abs(eta_r).astype(np.float32)).astype(np.float64)) + tenth * d_var + SUM_ROUNDING
            assert (np.abs(mean - N * pr) <= N * bar).all() and (np.abs(pvar - N * pr * (1.0 - pr)) <= N * bar).all()
        else:
            mr = np.exp(eta_in + 0.5 * var_r)
            ev = np.exp(var_r)
            vr = mr + mr * mr * np.expm1(var_r) + (mr * mr * ev / d["r"] if family == "negative_binomial" else 0.0)
            dm = d_eta + 0.5 * d_var                       # d log m
            extra = 1.0 + (1.0 / d["r"] if family == "negative_binomial" else 0.0)
            assert (np.abs(mean - mr) <= 2.0 * mr * dm + 16 * sref.EPS * mr).all()
            assert (np.abs(pvar - vr) <= 2.0 * ((mr + 2.0 * mr * mr * ev * extra) * dm + mr * mr * ev * extra * d_var) + 16 * sref.EPS * vr).all()


@pytest.mark.parametrize("family", sref.FAMILIES)
@pytest.mark.parametrize("case", FIXTURES)
def test_log_evidence_matches_function_space(mgp, golden, dev, case, family):
    """log_evidence() against the dense function-space Laplace evidence on K = s Z_obs Z_obs^T: 1e-6 of
    |sum l| + w.w / (2 s) + |logdet|, the bar of the CPU test"""
    M, c = _fit_case(mgp, golden, dev, case, family)
    dense = sref.dense_fit(M["Z64"], c["d"], M["s"], rtol=1e-12)
    got = c["fit"].log_evidence()
    print("%s %s: log Z %.10g, function space %.10g (%.1e of the scale)" % (case, family, got, dense["log_z"],
                                                                           abs(got - dense["log_z"]) / dense["scale"]))
    assert abs(got - dense["log_z"]) <= 1e-6 * dense["scale"]
    assert float(np.linalg.norm(dense["w"] - c["w_ref"])) <= sref.weight_bound(M["s"], [dense["grad"]], [c["bound"] / M["s"]])


def test_model_method(mgp, golden, dev):
    """RiemannGP.spectral_laplace_posterior: the fit of spectral_laplace_fit on features(train_x) with the model's outputscale;
    points and their feature rows predict alike; an error names eval() before it; a point far outside the bump support gets the
    prior's prediction."""
    from manifold_gp_amd.classification import bernoulli_predict
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.spectral_laplace import SpectralLaplaceFit
    M, c = _fit_case(mgp, golden, dev, "dumbbell_k10_loop", "bernoulli")
    g, model = M["g"], M["model"]
    obs = T(c["d"]["obs"], dev)
    model.train_targets = T(np.where(c["d"]["obs"], c["pub"]["y"], np.nan), dev, torch.float32)
    fit = model.spectral_laplace_posterior(obs)
    assert isinstance(fit, SpectralLaplaceFit) and fit.kernel is M["kern"] and fit.outputscale == M["s"]
    assert torch.equal(fit.weights, c["fit"].weights)
    x = T(g["test_x"], dev)
    for a, b in zip(fit.latent(x), fit.latent(M["Zs"])):
        assert torch.equal(a, b)
    assert torch.equal(fit.predict_proba(x), fit.predict_proba(M["Zs"]))
    with pytest.raises(ValueError, match="points or"):
        fit.latent(torch.zeros(3, 7, device=dev))
    with pytest.raises(ValueError, match="is the model's own"):
        model.spectral_laplace_posterior(obs, outputscale=2.0)
    # far outside the support: a zero feature row, eta = mean and var = 0 exactly
    far = torch.tensor([[100.0, 100.0]], device=dev)
    pois = model.spectral_laplace_posterior(obs, family="bernoulli", mean=0.75)
    eta, var = pois.latent(far)
    assert float(eta) == 0.75 and float(var) == 0.0
    prior = bernoulli_predict(torch.tensor([0.75], device=dev), torch.zeros(1, dtype=torch.float64, device=dev))
    assert torch.equal(pois.predict_proba(far), prior)
    # before eval(): no eigenpairs
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=5, laplacian_normalization="randomwalk", num_modes=4).to(dev)
    fresh = RiemannGP(x, torch.zeros(x.shape[0], device=dev), GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
    with pytest.raises(RuntimeError, match=r"eval\(\)"):
        fresh.spectral_laplace_posterior()
