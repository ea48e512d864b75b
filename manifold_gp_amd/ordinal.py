"""Ordered categories at the graph nodes: the Laplace approximation of a graph Matern GP with a cumulative-logit likelihood
(docs/kernels/ordinal.md).

K categories 0 .. K-1 with cutpoints b_1 < .. < b_{K-1} (b_0 = -inf, b_K = +inf) and ONE latent function f with the form-0
precision Q2 of sampling.py:  P(y <= k | f) = sigma(b_{k+1} - f).  At an observed node of category k, with lo = b_k, hi = b_{k+1},
u = hi - f and l = lo - f,

    P(y = k | f) = sigma(u) - sigma(l) = sigma(u) sigma(-l) (1 - exp(-(hi - lo)))          (the product form: no cancellation)
    g = d log p / df = sigma(l) - sigma(-u),     h = -d2 log p / df2 = sigma(u) sigma(-u) + sigma(l) sigma(-l)  in (0, 1/2]

(g = h = 0 elsewhere).  The likelihood is log-concave in f and the Hessian diagonal, so the mode of
psi(f) = sum_obs log p_i - 1/2 f^T Q2 f is found by the Newton loop of classification.py (_newton) with its gradient rule: a step
solves (H + Q2) delta = g - Q2 f, which multiplied by S_REF = 2 is operator form 3 with obs_w = 2 h in [0, 1] and noise = 2.  The
per-node stage is one kernel (mgp_ordinal_site), which takes the interval (lo, hi] per node and never a label; Q2 f comes from
the float64 chain (classification._q2); the solve is the library's Jacobi-preconditioned CG.  With K = 2 and b_1 = 0 this is the
Bernoulli-logit fit of classification.laplace_fit.

The cutpoints are fixed during the fit: the caller's, or the logits of the smoothed cumulative frequencies of the observed
labels (ordinal_cutpoints).  They are rounded to float32, the format the kernel reads them in, and the fit keeps those values.

The Laplace posterior N(f_hat, (Q2 + H)^-1) is the form-3 GMRF posterior with pseudo-noise 1 / h and pseudo-targets
f_hat + g / h: OrdinalLaplaceFit supplies (g, h) (families.TABLE) and inherits _pseudo, latent_variance / latent_samples.  The predictive probabilities
of the K categories come from one quadrature per (node, category) in float64 (mgp_ordinal_predict).

The Laplace evidence of the fit is evidence.laplace_evidence (OrdinalLaplaceFit.laplace_evidence) with the per-node stage
mgp_ordinal_evidence_site; its derivative with respect to the cutpoints is three per-cutpoint sums over the nodes
(mgp_ordinal_cut_sums).  CutpointParameter states strictly increasing cutpoints in unconstrained parameters and learn_cutpoints
runs Adam on them, one warm-started fit per step: the frequency logits are the right cutpoints for a flat latent function only.
"""
import torch

from . import _lib, _sites, sampling
from ._lib import check, lib, ptr, stream
from .classification import H_FLOOR, LaplaceFit, _newton_form3, _points
from .counts import CountLaplaceFit
from ._sites import check_mask
from .families import TABLE, _sig, _widths

MAX_CATEGORIES = 64
S_REF = 2.0              # obs_w = S_REF h <= 1
MIN_GAP = 2.0 ** -20     # the least distance of two cutpoints a fit takes


def _categories(num_categories):
    if isinstance(num_categories, bool) or not isinstance(num_categories, int) or not 2 <= num_categories <= MAX_CATEGORIES:
        raise ValueError("num_categories must be an int in 2 .. %d, got %r" % (MAX_CATEGORIES, num_categories))
    return num_categories


def _labels(y, n, K, mask, what):
    """y [n] with integers in [0, K) where mask (None: everywhere) holds: int64 on y's device, 0 at the other nodes"""
    if not torch.is_tensor(y) or y.numel() != n or y.dtype == torch.bool or y.is_complex():
        raise ValueError("y must be a tensor of %d categories, got %s" % (n, tuple(y.shape) if torch.is_tensor(y) else type(y)))
    y = y.reshape(-1)
    mask = None if mask is None else mask.to(y.device)
    seen = y if mask is None else y[mask]
    whole = (seen == seen.round()) if seen.is_floating_point() else torch.ones_like(seen, dtype=torch.bool)
    if not bool(((seen >= 0) & (seen < K) & whole).all()):
        raise ValueError("categories at the %s nodes must all be integers in [0, %d)" % (what, K))
    if y.is_floating_point():
        y = torch.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0).clamp(0.0, float(K - 1))
    y = y.to(torch.int64).clamp(0, K - 1)
    return y if mask is None else torch.where(mask, y, torch.zeros_like(y))


def _cutpoints(cutpoints, K=None, min_gap=0.0):
    """The K - 1 cutpoints as a float64 tensor on the host: a real tensor of finite, strictly increasing values (gaps >= min_gap)"""
    if (not torch.is_tensor(cutpoints) or cutpoints.dtype == torch.bool or cutpoints.is_complex() or cutpoints.dim() != 1
            or not 1 <= cutpoints.shape[0] < MAX_CATEGORIES or (K is not None and cutpoints.shape[0] != K - 1)):
        raise ValueError("cutpoints must be a real tensor of %s values, got %s"
                         % ("1 .. %d" % (MAX_CATEGORIES - 1) if K is None else "%d" % (K - 1),
                            tuple(cutpoints.shape) if torch.is_tensor(cutpoints) else type(cutpoints)))
    b = cutpoints.detach().to("cpu", torch.float64)
    if not bool(torch.isfinite(b).all()):
        raise ValueError("cutpoints must be finite")
    gaps = b[1:] - b[:-1]
    if not bool((gaps > 0.0).all()):
        raise ValueError("cutpoints must be strictly increasing")
    if not bool((gaps >= min_gap).all()):
        raise ValueError("cutpoints must lie at least 2^-20 apart, got a gap of %g" % float(gaps.min()))
    return b


def ordinal_cutpoints(y, num_categories, observed=None):
    """Cutpoints from the labels: float64 [K - 1] on the host, b_k = logit(sum_{j < k} (n_j + 1/2) / (N + K / 2)), the logits of the
    cumulative frequencies of the N observed labels with half a count added to every category -- strictly increasing with
    empty categories too.  y [n] integers in [0, K) at the observed nodes (bool [n]; None: every node; NaN allowed elsewhere).
    Host arithmetic: the numerator and 1 - it are both sums of positive counts."""
    K = _categories(num_categories)
    if not torch.is_tensor(y) or y.dim() != 1:
        raise ValueError("y must be a tensor [n] of categories")
    n = y.shape[0]
    observed = check_mask(observed, n)
    labels = _labels(y, n, K, observed, "observed").cpu()
    if observed is not None:
        labels = labels[observed.cpu()]
    mass = torch.bincount(labels, minlength=K).to(torch.float64) + 0.5
    below = mass.cumsum(0)[:-1]
    above = mass.flip(0).cumsum(0).flip(0)[1:]
    return torch.log(below) - torch.log(above)


def ordinal_site(f, qf, lo, hi, observed=None, s_ref=S_REF):
    """(w, rhs, sums) of mgp_ordinal_site: w = s_ref h and rhs = s_ref (g - qf) as fresh float32 [n] tensors, sums [4] float64 on
    the device (sum_obs (log sigma(hi - f) + log sigma(f - lo)), sum f qf, max |g - qf|, sum (g - qf)^2; the f-independent
    sum_obs log(1 - exp(-(hi - lo))) is the caller's).  f [n] float32; qf [n] or None (zeros); lo, hi [n] float32: the ends of
    every node's interval of cutpoints, lo < hi, -inf / +inf at the end categories, read at observed nodes only (NaN allowed
    elsewhere); observed [n] bool or None (every node)."""
    f, qf, (lo, hi), observed, n, w, rhs, sums, work = _sites.newton_args(
        f, qf, (("lo", lo), ("hi", hi)), (), observed, "ordinal_site", lib().mgp_ordinal_site_workspace_bytes)
    check(lib().mgp_ordinal_site(ptr(f), ptr(qf), ptr(lo), ptr(hi), ptr(observed), n, float(s_ref), ptr(w), ptr(rhs), ptr(sums),
                                 ptr(work), work.numel(), stream()), "mgp_ordinal_site")
    return w, rhs, sums


def ordinal_evidence_site(f, lo, hi, observed=None, variance=None, h_floor=H_FLOOR):
    """(root_h, corr, sums) of mgp_ordinal_evidence_site at the mode f [n] float32, the contract of evidence.evidence_site with the
    intervals (lo, hi] of ordinal_site in the place of the observations: root_h = sqrt(h) and corr = variance h' as fresh float32
    [n] tensors (0 off the observed nodes with h >= h_floor; corr None when variance is None), sums [4] float64 on the device
    (sum_obs (log sigma(hi - f) + log sigma(f - lo)), m = nodes kept, sum corr, max |corr|).  variance [n] (taken as float64)."""
    f, (lo, hi), observed, variance, n, root_h, corr, sums, work = _sites.evidence_args(
        f, (("lo", lo), ("hi", hi)), (), observed, variance, h_floor, lib().mgp_ordinal_evidence_site_workspace_bytes)
    check(lib().mgp_ordinal_evidence_site(ptr(f), ptr(lo), ptr(hi), ptr(observed), ptr(variance), n, float(h_floor), ptr(root_h),
                                          ptr(corr), ptr(sums), ptr(work), work.numel(), stream()), "mgp_ordinal_evidence_site")
    return root_h, corr, sums


def ordinal_cut_sums(f, lo, hi, cat, observed, variance, u, K, h_floor=H_FLOOR):
    """The three rows of d log Z / d b_k, k = 1 .. K - 1 (mgp_ordinal_cut_sums): [3, K - 1] float64 on the device -- the
    likelihood's term, the curvature's at fixed f (zeros when variance is None) and the one through the mode (zeros when u is
    None); their column sum is the derivative.  f [n] float32: the mode; lo, hi [n] as ordinal_site; cat [n]: the category of
    every node, an integer tensor (uint8 as it is, any other integer type with values outside 0 .. 255 set to 255), read at
    observed nodes only, a value >= K adds nothing; observed [n] bool or None; variance [n]: diag(A^-1) and u [n]:
    A^-1 (variance o h'), taken as float64."""
    K = _categories(K)
    if not torch.is_tensor(cat) or cat.dtype == torch.bool or cat.is_floating_point() or cat.is_complex():
        raise ValueError("cat must be an integer tensor [n] of categories")
    n = _sites.check_evidence_args(f, (("lo", lo), ("hi", hi)), (), observed, variance, h_floor, (("cat", cat), ("u", u)))
    _lib.require_device(f, lo, hi, cat, observed, variance, u)
    f, lo, hi = _lib.f32c(f.reshape(-1)), _lib.f32c(lo.reshape(-1)), _lib.f32c(hi.reshape(-1))
    cat = cat.reshape(-1)
    if cat.dtype != torch.uint8:
        cat = torch.where((cat < 0) | (cat > 255), torch.full_like(cat, 255), cat).to(torch.uint8)
    cat = cat.contiguous()
    observed = None if observed is None else observed.reshape(-1).contiguous()
    variance = None if variance is None else variance.reshape(-1).to(torch.float64).contiguous()
    u = None if u is None else u.reshape(-1).to(torch.float64).contiguous()
    out = torch.empty((3, K - 1), dtype=torch.float64, device=f.device)
    work = _lib.workspace(lib().mgp_ordinal_cut_sums_workspace_bytes(n, K), "ordinal_cut_sums", f.device)
    check(lib().mgp_ordinal_cut_sums(ptr(f), ptr(lo), ptr(hi), ptr(cat), ptr(observed), ptr(variance), ptr(u), n, K, float(h_floor),
                                     ptr(out), ptr(work), work.numel(), stream()), "mgp_ordinal_cut_sums")
    return out


GAP_FLOOR = 2.0 ** -10   # the least gap of a CutpointParameter: distinct after the fit's float32 rounding for |b| < 2^12


class CutpointParameter(torch.nn.Module):
    """K - 1 strictly increasing cutpoints as a differentiable function of unconstrained float64 parameters
    raw = (b_1, rho_2 .. rho_{K-1}):  forward() = b_1, b_1 + sum_{j <= k} (2^-10 + softplus(rho_j)).  init [K - 1]: the start, for
    example ordinal_cutpoints(...), reproduced up to rounding; its gaps must exceed 2^-10."""

    def __init__(self, num_categories, init):
        super().__init__()
        K = _categories(num_categories)
        b = _cutpoints(init, K)
        x = b[1:] - b[:-1] - GAP_FLOOR
        if not bool((x > 0.0).all()):
            raise ValueError("the cutpoints of a CutpointParameter must lie more than 2^-10 apart, got a gap of %g"
                             % float((b[1:] - b[:-1]).min()))
        rho = x + torch.log(-torch.expm1(-x))                 # the inverse of softplus: log(expm1(x)), no overflow
        self.num_categories = K
        self.raw = torch.nn.Parameter(torch.cat([b[:1], rho]))

    def forward(self):
        gaps = GAP_FLOOR + torch.nn.functional.softplus(self.raw[1:])
        return self.raw[0] + torch.cat([torch.zeros_like(self.raw[:1]), gaps.cumsum(0)])


def _live_cutpoints(fit_kw):
    """(fit_kw with cutpoints detached, the live tensor or None): cutpoints given as a CutpointParameter are evaluated now; a
    tensor that requires grad, theirs or the caller's, is what laplace_evidence differentiates."""
    fit_kw = dict(fit_kw)
    c = fit_kw.get("cutpoints")
    if isinstance(c, torch.nn.Module):
        c = c()
    if not torch.is_tensor(c):
        return fit_kw, None
    fit_kw["cutpoints"] = c.detach()
    return fit_kw, (c if c.requires_grad else None)


def learn_cutpoints(desc, y, num_categories, observed=None, cutpoints0=None, steps=30, lr=0.1, var_samples=64, variance=None,
                    fit_kw=None, evidence_kw=None):
    """Learn the cutpoints on the Laplace evidence with the kernel hyper-parameters fixed: Adam(lr) for `steps` steps on a
    CutpointParameter started at cutpoints0 (None: ordinal_cutpoints of the observed labels), loss -log Z / m, every fit
    warm-started from the previous mode, the gradient that of evidence.laplace_evidence(cutpoints=).  variance: None (every
    step draws fit.latent_variance(var_samples)[0]), or a callable fit -> diag(A^-1) [n].  fit_kw as laplace_fit_ordinal takes,
    evidence_kw as laplace_evidence.  Returns (cutpoints float64 [K - 1] on the device, as float32 holds them; the
    OrdinalLaplaceFit at them; history: one (log Z, se) per step, taken before the step's update)."""
    from .evidence import laplace_evidence
    K = _categories(num_categories)
    steps = _sites.learning_args(steps, lr, variance)
    fit_kw, evidence_kw = dict(fit_kw or {}), dict(evidence_kw or {})
    if cutpoints0 is None:
        labels, mask, _ = _validate(desc, y, K, None, observed, None)
        cutpoints0 = ordinal_cutpoints(labels, K, None if mask is None else mask.to(labels.device))
    cut = CutpointParameter(K, cutpoints0)
    opt = torch.optim.Adam(cut.parameters(), lr=float(lr))
    f0, history = fit_kw.pop("f0", None), []
    for _ in range(steps):
        opt.zero_grad()
        b = cut()
        fit = laplace_fit_ordinal(desc, y, K, b.detach(), observed, f0=f0, **fit_kw)
        f0 = fit.mean
        ev = laplace_evidence(fit, variance=None if variance is None else variance(fit), var_samples=var_samples, cutpoints=b,
                              **evidence_kw)
        history.append((float(ev.value.detach()), ev.se))
        (-ev.value / ev.m).backward()
        opt.step()
    fit = laplace_fit_ordinal(desc, y, K, cut().detach(), observed, f0=f0, **fit_kw)
    return fit.cutpoints.clone(), fit, history


def ordinal_predict(eta, var, cutpoints, points=129, log=False):
    """P(y = k) = int P(y = k | f) N(f; eta_i, var_i) df for the K = len(cutpoints) + 1 categories at every node: [n, K] float64
    (mgp_ordinal_predict), its log with log=True.  eta, var [n] (taken as float64; var <= 2^-76, negative entries included: the
    plain probability at eta); cutpoints [K - 1] strictly increasing (checked on the host); points: the odd number of nodes
    of the trapezoid rule on [-8, 8], 9 .. 1025.  Rows sum to 1."""
    points = _points(points)
    b = _cutpoints(cutpoints)
    _lib.require_device(eta, var)
    eta = eta.reshape(-1).to(torch.float64).contiguous()
    var = var.reshape(-1).to(torch.float64).contiguous()
    if var.shape[0] != eta.shape[0]:
        raise ValueError("var has %d entries, eta %d" % (var.shape[0], eta.shape[0]))
    n, K = eta.shape[0], b.shape[0] + 1
    cuts = cutpoints.detach().to(eta.device, torch.float64).contiguous()
    out = torch.empty((n, K), dtype=torch.float64, device=eta.device)
    check(lib().mgp_ordinal_predict(ptr(eta), ptr(var), ptr(cuts), n, K, points, int(bool(log)), ptr(out), stream()),
          "mgp_ordinal_predict")
    return out


def _validate(desc, y, num_categories, cutpoints, observed, f0):
    """The host-side argument checks of laplace_fit_ordinal, before any device call: the descriptor's, check_data and the start's"""
    sampling._check_desc(desc)
    checked = check_data(desc.n, y, num_categories, cutpoints, observed)
    if f0 is not None and (not torch.is_tensor(f0) or f0.numel() != desc.n):
        raise ValueError("f0 must be a tensor of %d latent values" % desc.n)
    return checked


def check_data(n, y, num_categories, cutpoints, observed):
    """The categories and the cutpoints of n nodes (or rows of features).  Returns (labels int64 [n] on y's device with 0 at
    unobserved nodes, observed, cutpoints float64 [K - 1] on the host as float32 holds them)."""
    K = _categories(num_categories)
    if torch.is_tensor(y) and y.numel() == n:
        y = y.reshape(-1)
    observed = check_mask(observed, n)
    labels = _labels(y, n, K, observed, "observed")
    if cutpoints is None:
        cutpoints = ordinal_cutpoints(labels, K, None if observed is None else observed.to(labels.device))
    b = _cutpoints(cutpoints, K, MIN_GAP)
    b32 = b.float().double()
    if not bool(torch.isfinite(b32).all()) or not bool((b32[1:] > b32[:-1]).all()):
        raise ValueError("cutpoints must stay finite and strictly increasing when rounded to float32")
    return labels, observed, b32


class OrdinalLaplaceFit(LaplaceFit):
    """The Laplace approximation N(mean, (Q2 + H)^-1) of the latent posterior given ordered categories (laplace_fit_ordinal).
    mean [n] float32: the mode f_hat; converged, iterations; history: one (psi, relative gradient, step, CG iterations) per
    Newton step, psi without the likelihood's f-independent factor; log_likelihood: sum_obs log P(y_i | f_hat_i) with it;
    y [n] int64: the labels, 0 at unobserved nodes; cutpoints [K - 1] float64 on the device, the values the fit used (the
    caller's rounded to float32); num_categories."""
    family, s_ref = "ordinal", S_REF

    def __init__(self, desc, y, observed, mean, converged, iterations, history, log_likelihood, cutpoints, lo, hi):
        super().__init__(desc, y, observed, mean, converged, iterations, history, log_likelihood)
        self.cutpoints, self.num_categories = cutpoints, int(cutpoints.shape[0]) + 1
        self._lo, self._hi = lo, hi           # what the kernel read: float32 [n], the interval of category 0 at unobserved nodes

    def _gh(self, f, obs):
        return TABLE[self.family].gh(f, self._lo.double(), self._hi.double(), None)

    def _weights(self):
        return ordinal_site(self.mean, None, self._lo, self._hi, self.observed, self.s_ref)[0]

    def evidence(self, **kw):
        raise NotImplementedError("the evidence of the ordinal fit is OrdinalLaplaceFit.laplace_evidence(...) or "
                                  "evidence.laplace_evidence(fit, ...): see docs/kernels/ordinal.md")

    def laplace_evidence(self, **kw):
        """The Laplace approximation of log p(y) at this mode, an evidence.LaplaceEvidence; kw as evidence.laplace_evidence
        (operator= for the hyper-parameter gradient, cutpoints= for the cutpoints', num_probes, steps, seed, method, ...)."""
        from .evidence import laplace_evidence
        return laplace_evidence(self, **kw)

    def map_proba(self):
        """P(y = k | f_hat) in the product form: the category probabilities at the mode, [n, K] float64 (ignores the latent
        variance)."""
        f = self.mean.double()[:, None]
        inf = torch.full((1,), float("inf"), dtype=torch.float64, device=f.device)
        below = _sig(torch.cat([self.cutpoints, inf])[None, :] - f)[0]
        above = _sig(f - torch.cat([-inf, self.cutpoints])[None, :])[0]
        return _widths(self.cutpoints)[None, :] * below * above

    _variance = CountLaplaceFit._variance

    def predict_proba(self, S=64, seed=None, points=129, variance=None, log=False):
        """(p, latent_var): P(y_new = k) for the K categories at every node under the Laplace posterior, [n, K] float64 (its log
        with log=True; rows of p sum to 1), and the latent marginal variance it used [n]: `variance` (a latent_variance result)
        or latent_variance(S, seed)[0].  One quadrature per (node, category) with `points` nodes (ordinal_predict)."""
        points = _points(points)
        v = self._variance(variance, S, seed)
        return ordinal_predict(self.mean.double(), v, self.cutpoints, points, log), v

    def predict_log_density(self, y, at=None, S=64, seed=None, points=129, variance=None):
        """log P(y_new = y_i) at the nodes of the bool mask at [n] (None: every node) under the Laplace posterior, float64 [n],
        NaN elsewhere: the log predictive density of held-out categories.  y [n]: integers in [0, K) at those nodes; not read
        elsewhere (NaN allowed)."""
        points = _points(points)
        n = self.mean.shape[0]
        at = check_mask(at, n, "at")
        labels = _labels(y, n, self.num_categories, at, "asked")
        _lib.require_device(y, at)
        logp = self.predict_proba(S, seed, points, variance, log=True)[0]
        picked = logp.gather(1, labels.to(logp.device)[:, None])[:, 0]
        if at is None:
            return picked
        return torch.where(at.to(logp.device), picked, torch.full_like(picked, float("nan")))

    def predict_exceedance(self, k, S=64, seed=None, points=129, variance=None):
        """P(y_new > k) at every node, float64 [n]: the sum of the probabilities of the categories above k (every term is
        positive: no 1 - cdf).  k: an int or an integer tensor [n], 0 .. K - 1."""
        points = _points(points)
        n, K = self.mean.shape[0], self.num_categories
        thr, top = _sites.threshold(k, n, "k", K - 1)
        p = self.predict_proba(S, seed, points, variance)[0]
        ks = torch.arange(K, device=p.device)[None, :]
        above = ks > (top if thr is None else thr.to(p.device)[:, None])
        return torch.where(above, p, torch.zeros((), dtype=p.dtype, device=p.device)).sum(1)

    def predict_category(self, kind="mode", S=64, seed=None, points=129, variance=None):
        """The predicted category at every node, int64 [n]: the most probable one (kind "mode") or the median of the predictive
        distribution, the least k with P(y_new <= k) >= 1/2 (kind "median")."""
        if kind not in ("mode", "median"):
            raise ValueError("kind must be 'mode' or 'median', got %r" % (kind,))
        points = _points(points)
        p = self.predict_proba(S, seed, points, variance)[0]
        if kind == "mode":
            return p.argmax(1)
        return (p.cumsum(1) < 0.5).sum(1).clamp_max(self.num_categories - 1)


def laplace_fit_ordinal(desc, y, num_categories, cutpoints=None, observed=None, rtol=1e-5, max_newton=30, cg_tol=1e-3,
                        max_iter=5000, f0=None):
    """The mode of the latent posterior given ordered categories y [n] in [0, num_categories) at the observed nodes (bool [n];
    None: every node; an integer tensor or a float tensor of whole numbers; the other entries are not read and may be NaN)
    under the cumulative-logit likelihood P(y <= k | f) = sigma(b_{k+1} - f), by Newton's method with step halving:
    OrdinalLaplaceFit.  num_categories: 2 .. 64.  cutpoints [num_categories - 1]: finite, strictly increasing, at least 2^-20
    apart, fixed during the fit and rounded to float32 (None: ordinal_cutpoints of the observed labels).
    desc: a form-0 precision descriptor as the samplers take.  Stops when max |g - Q2 f| <= rtol times its value at f = 0
    (|g| <= 1, as for 0/1 labels); every step is a form-3 CG solve to the relative residual cg_tol.  f0 [n]: the start
    (default 0)."""
    labels, observed, b = _validate(desc, y, num_categories, cutpoints, observed, f0)
    _lib.require_device(labels, f0)
    dev = desc.data.graph.device
    labels = labels.to(dev)
    obs = None if observed is None else observed.to(dev).contiguous()
    b = b.to(dev)
    inf = torch.full((1,), float("inf"), dtype=torch.float64, device=dev)
    lo = torch.cat([-inf, b])[labels].float().contiguous()
    hi = torch.cat([b, inf])[labels].float().contiguous()
    widths = TABLE["ordinal"].constant(labels, None, b)
    const = float((widths if obs is None else widths[obs]).sum())
    f, sums, converged, its, history = _newton_form3("laplace_fit_ordinal", desc, lambda f, qf: ordinal_site(f, qf, lo, hi, obs, S_REF),
                                                     S_REF, f0, rtol, max_newton, cg_tol, max_iter)
    return OrdinalLaplaceFit(desc, labels, obs, f, converged, its, history, sums[0] + const, b, lo, hi)
