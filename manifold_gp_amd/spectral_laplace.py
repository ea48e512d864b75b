"""Laplace fits on the spectral features: the five node families at points that were not in the graph
(docs/kernels/spectral_laplace.md).

The precision-form fits (classification.py, counts.py, ordinal.py) live on the n graph nodes.  Taken through the spectral kernel
K = s Z Z^T of the regression side (RiemannMaternKernel.features) the same model has m <= 512 unknowns: f = Z w + mean with
w ~ N(0, s I_m), and

    psi(w) = sum_obs l_i(z_i . w + mean) - w . w / (2 s),    grad = Z^T g - w / s,    A = Z^T diag(h) Z + I / s    (A >= I / s)
    Newton:  A delta = grad, step halving on psi;      at x*:  eta* = z* . w_hat + mean,   var* = z*^T A^-1 z*
    log Z ~= sum_obs l_i(f_hat_i) + constants - w_hat . w_hat / (2 s) - 1/2 logdet(s A)

all of it closed-form m x m float64 algebra: no CG, no sampled variance, no Lanczos quadrature.  The pass over Z that forms the
latent values, the likelihood terms, Z^T g and the weighted Gram is one entry point, mgp_spectral_site (spectral_site); the
m x m Cholesky and solves are torch on the device.  The predictive quadratures are the stand-alone functions of the node fits
(bernoulli_predict, count_predict_pmf / count_predict_logpmf, ordinal_predict) on rows of Z* in place of nodes.

A test point outside the bump support has a zero feature row: eta = mean and var = 0, the prior's answer at a point the kernel
does not reach.  A NaN feature row (mgp_features_oos: a point inside the support whose neighbour weights all underflow) gives NaN
predictions.
"""
import math
import warnings

import torch

from . import _lib, families
from ._lib import check, lib, ptr, stream
from .classification import MAX_HALVINGS, _points, bernoulli_predict
from .counts import PMF_POINTS, count_predict_logpmf, count_predict_pmf
from ._sites import _node_vector, _real
from .ordinal import _labels, check_data as _check_categories, ordinal_predict

FAMILIES = families.codes("spectral")
COUNT_FAMILIES = tuple(sorted(families.codes("count"), key=families.codes("count").get))
MAX_MODES = 512              # the cap of mgp_spectral_site (and of mgp_gram_f64)
# A trial point is taken when psi does not decrease beyond the rounding of its two terms: both are float64 sums of at most
# n + m terms, SLACK of their size covers 2^13 ulps
SLACK = 2.0 ** -40


def _features(Z, name="Z"):
    """(n, m) of a feature block: a real 2-D tensor with 1 <= m <= 512 columns and at least one row"""
    if not torch.is_tensor(Z) or Z.dim() != 2 or not Z.is_floating_point():
        raise ValueError("%s must be a float tensor [n, m] of feature rows, got %s"
                         % (name, tuple(Z.shape) if torch.is_tensor(Z) else type(Z)))
    n, m = Z.shape
    if n < 1:
        raise ValueError("%s has no rows" % name)
    if not 1 <= m <= MAX_MODES:
        raise ValueError("%s has %d columns: the spectral Laplace fit takes 1 .. %d modes" % (name, m, MAX_MODES))
    return n, m


def _mean(mean):
    mean = _real(mean, "mean")
    if not math.isfinite(mean):
        raise ValueError("mean must be finite, got %r" % (mean,))
    return mean


def spectral_site(Z, w, family, a, b=None, observed=None, mean=0.0, dispersion=None, hessian=True):
    """(f, grad, hess, sums) of mgp_spectral_site, fresh float64 tensors on the device: f [n] = Z w (without mean), grad [m] =
    Z^T g, hess [m, m] = Z^T diag(h) Z (None with hessian=False: a line-search evaluation), sums [2] = (sum_obs l without the
    families' constants, max |f|); the prior's terms are the caller's.  Z [n, m] float32 (m <= 512; a view at any alignment is
    read in place), w [m] (taken as float64); family one of FAMILIES; a, b [n] float32, read at observed rows only (NaN
    allowed elsewhere): labels (bernoulli), counts and log-exposure or None (poisson, negative_binomial with dispersion=),
    counts and trials (binomial), the ends (lo, hi] of the row's interval of cutpoints (ordinal); observed [n] bool or None
    (every row); mean: the constant added to f inside the likelihood."""
    rec = families._family(family, "spectral")
    n, m = _features(Z)
    r = families.check_dispersion(rec, dispersion)
    if rec.aux in ("trials", "interval") and b is None:
        raise ValueError("the binomial family needs the trials in b" if rec.aux == "trials"
                         else "the ordinal family needs the upper cutpoints in b")
    mean = _mean(mean)
    if not torch.is_tensor(w) or w.numel() != m or not w.is_floating_point():
        raise ValueError("w must be a float tensor of %d weights" % m)
    for name, t in (("a", a), ("b", b)):
        if t is not None and (not torch.is_tensor(t) or t.numel() != n):
            raise ValueError("%s must be a tensor of %d values" % (name, n))
    if a is None:
        raise ValueError("a must be a tensor of %d values" % n)
    if observed is not None and (not torch.is_tensor(observed) or observed.dtype != torch.bool or observed.numel() != n):
        raise ValueError("observed must be a bool tensor [%d]" % n)
    _lib.require_device(Z, w, a, b, observed)
    Z = _lib.f32c(Z)
    w = w.reshape(-1).to(torch.float64).contiguous()
    a = _lib.f32c(a.reshape(-1))
    b = None if b is None else _lib.f32c(b.reshape(-1))
    observed = None if observed is None else observed.reshape(-1).contiguous()
    dev = Z.device
    f = torch.empty(n, dtype=torch.float64, device=dev)
    grad = torch.empty(m, dtype=torch.float64, device=dev)
    hess = torch.empty((m, m), dtype=torch.float64, device=dev) if hessian else None
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    nbytes = lib().mgp_spectral_site_workspace_bytes(n, m, int(bool(hessian)))
    work = _lib.workspace(nbytes, "spectral_site", dev)
    check(lib().mgp_spectral_site(ptr(Z), n, m, ptr(w), rec.spectral, ptr(a), ptr(b), ptr(observed), mean, 0.0 if r is None else r, ptr(f),
                                  ptr(grad), ptr(hess), ptr(sums), ptr(work), work.numel(), stream()), "mgp_spectral_site")
    return f, grad, hess, sums


class SpectralLaplaceFit:
    """The Laplace approximation of the posterior of the weights, N(weights, A^-1) with A = Z^T H Z + I / s
    (spectral_laplace_fit).  weights [m] float64: the mode w_hat; chol [m, m] float64: the lower Cholesky factor of A at the
    mode; mean [n] float64: the latent function Z w_hat + prior_mean at the training rows; converged, iterations; history: one
    (psi, relative gradient, step) per Newton step, psi without the likelihood's constants; log_likelihood: sum_obs
    log p(y_i | mean_i) with them; family, outputscale, prior_mean, dispersion (negative binomial), cutpoints [K - 1] float64 on
    the device and num_categories (ordinal); kernel: the RiemannMaternKernel the fit is bound to
    (RiemannGP.spectral_laplace_posterior) or None.

    The predict methods take the feature rows Zs [T, m] of the test points; a fit bound to a kernel also takes the points
    themselves, x [T, d], and calls kernel.features(x) (a [T, k] input is read as points when k = d, as features when k = m != d).
    A zero feature row (a point outside the bump support) gets eta = prior_mean and var = 0; a NaN row gets NaN."""

    def __init__(self, weights, chol, mean, converged, iterations, history, log_likelihood, family, outputscale, prior_mean,
                 dispersion=None, cutpoints=None, kernel=None):
        self.weights, self.chol, self.mean = weights, chol, mean
        self.converged, self.iterations, self.history, self.log_likelihood = converged, iterations, history, log_likelihood
        self.family, self.outputscale, self.prior_mean, self.dispersion = family, outputscale, prior_mean, dispersion
        self.cutpoints = cutpoints
        self.num_categories = None if cutpoints is None else int(cutpoints.shape[0]) + 1
        self.kernel = kernel

    # ------------------------------------------------------------------------------------------------ the latent function
    def _rows(self, Zs):
        m = self.weights.shape[0]
        if not torch.is_tensor(Zs) or Zs.dim() != 2 or not Zs.is_floating_point() or Zs.shape[0] < 1:
            raise ValueError("expected a float tensor [T, %d] of feature rows%s, got %s"
                             % (m, "" if self.kernel is None else " or [T, d] of points",
                                tuple(Zs.shape) if torch.is_tensor(Zs) else type(Zs)))
        if self.kernel is not None:
            d = self.kernel.knn.x.shape[1]
            if Zs.shape[1] == d:
                _lib.require_device(Zs)
                Zs = self.kernel.features(_lib.f32c(Zs))
            elif Zs.shape[1] != m:
                raise ValueError("expected [T, %d] points or [T, %d] feature rows, got %s" % (d, m, tuple(Zs.shape)))
        elif Zs.shape[1] != m:
            raise ValueError("expected [T, %d] feature rows, got %s" % (m, tuple(Zs.shape)))
        _lib.require_device(Zs)
        return Zs.to(self.weights.device, torch.float64)

    def latent(self, Zs):
        """(eta, var): the latent function z* . w_hat + prior_mean at the test rows and its variance z*^T A^-1 z*, float64 [T]
        each."""
        Zd = self._rows(Zs)
        eta = Zd @ self.weights + self.prior_mean
        half = torch.linalg.solve_triangular(self.chol, Zd.T, upper=False)          # L^-1 z*: var = |L^-1 z*|^2 >= 0
        return eta, (half * half).sum(0)

    def _only(self, families, what):
        if self.family not in families:
            raise NotImplementedError("a %s fit has no %s" % (self.family, what))

    # ------------------------------------------------------------------------------------------------ classes
    def predict_proba(self, Zs, points=129, log=False):
        """bernoulli: the class-1 probability int sigma(f) N(f; eta, var) df, float64 [T] (bernoulli_predict; eta as float32, its
        input format); ordinal: P(y = k) for the K categories, [T, K] (ordinal_predict; its log with log=True)."""
        self._only(("bernoulli", "ordinal"), "class probability: see predict_mean and predict_pmf")
        points = _points(points)
        eta, var = self.latent(Zs)
        if self.family == "ordinal":
            return ordinal_predict(eta, var, self.cutpoints, points, log)
        p = bernoulli_predict(eta, var, points)
        return p.log() if log else p

    # ------------------------------------------------------------------------------------------------ counts
    def _aux(self, T, exposure, trials, dev):
        """(log-exposure float64 [T] or None, trials float32 [T] or None) of T test rows; ones where none is given"""
        extra = families.check_aux(families.TABLE[self.family], T, exposure, trials)
        _lib.require_device(exposure, trials)
        if self.family == "binomial":
            return None, torch.ones(T, dtype=torch.float32, device=dev) if extra is None else extra.to(dev).float()
        return None if extra is None else extra.to(dev).log(), None

    def _count_args(self, Zs, exposure, trials):
        eta, var = self.latent(Zs)
        log_e, N = self._aux(eta.shape[0], exposure, trials, eta.device)
        return (eta if log_e is None else eta + log_e), var, N                     # the log-exposure added in float64

    def predict_mean(self, Zs, exposure=None, trials=None, points=129):
        """(mean, var): the mean and the variance of a new count at the test rows, float64 [T] each, by the formulas of
        CountLaplaceFit.predict_mean: closed form for the Poisson and negative-binomial families (the rate is log-normal), the
        quadrature of bernoulli_predict for the binomial.  exposure / trials [T]: the test rows' own (None: ones)."""
        self._only(COUNT_FAMILIES, "expected count: see predict_proba")
        points = _points(points)
        eta, v, N = self._count_args(Zs, exposure, trials)             # (the exposure is in eta)
        return families.count_moments(families.TABLE[self.family], eta, v, None if N is None else N.double(), self.dispersion,
                                      points)

    def predict_pmf(self, Zs, kmax, kmin=0, exposure=None, trials=None, points=PMF_POINTS, log=False):
        """P(y_new = k) for k = kmin .. kmax at the test rows, [T, kmax - kmin + 1] float64 (its log with log=True):
        count_predict_pmf on (eta, var)."""
        self._only(COUNT_FAMILIES, "pmf of counts: see predict_proba")
        eta, v, N = self._count_args(Zs, exposure, trials)
        return count_predict_pmf(eta, v, N, self.family, kmin, kmax, points, log, self.dispersion)

    def predict_log_density(self, Zs, y, exposure=None, trials=None, points=None):
        """log P(y_new = y_i) at the test rows, float64 [T]: held-out labels (bernoulli: 0 / 1), categories (ordinal: integers in
        [0, K)) or counts (count_predict_logpmf; at most the trials for the binomial family)."""
        if self.family in COUNT_FAMILIES:
            eta, v, N = self._count_args(Zs, exposure, trials)
            T = eta.shape[0]
            y = _node_vector(y, T, "y")
            if not bool(((y >= 0) & (y <= 2 ** 24) & (y == y.round())).all()):
                raise ValueError("counts must all be integers in [0, 2^24]")
            if N is not None and not bool((y.to(N.device) <= N.double()).all()):
                raise ValueError("counts must be at most the trials")
            return count_predict_logpmf(eta, v, N, y.to(eta.device), None, self.family, PMF_POINTS if points is None else points,
                                        self.dispersion)
        if exposure is not None or trials is not None:
            raise ValueError("exposure and trials belong to the count families")
        p = self.predict_proba(Zs, 129 if points is None else points, log=self.family == "ordinal")
        T = p.shape[0]
        if self.family == "ordinal":                                               # p holds the logs
            labels = _labels(y, T, self.num_categories, None, "asked")
            return p.gather(1, labels.to(p.device)[:, None])[:, 0]
        if not torch.is_tensor(y) or y.numel() != T or not bool(((y == 0) | (y == 1)).all()):
            raise ValueError("y must be a tensor of %d labels, all 0 or 1" % T)
        one = y.reshape(-1).to(p.device) > 0.5
        return torch.where(one, p.log(), torch.log1p(-p))

    # ------------------------------------------------------------------------------------------------ the evidence
    def log_evidence(self):
        """The Laplace approximation of log p(y): log_likelihood - w_hat . w_hat / (2 s) - 1/2 logdet(s A), a float.
        log_likelihood carries the families' constants as evidence.LaplaceEvidence.log_likelihood does."""
        m = self.weights.shape[0]
        s = self.outputscale
        logdet = m * math.log(s) + 2.0 * float(torch.log(self.chol.diagonal()).sum())
        return self.log_likelihood - 0.5 * float(self.weights.dot(self.weights)) / s - 0.5 * logdet


def _check_fit_args(Z, outputscale, mean, rtol, max_newton, w0):
    n, m = _features(Z)
    s = _real(outputscale, "outputscale")
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError("outputscale must be finite and positive, got %r" % (outputscale,))
    mean = _mean(mean)
    if not _real(rtol, "rtol") > 0.0:
        raise ValueError("rtol must be positive, got %r" % (rtol,))
    if isinstance(max_newton, bool) or not isinstance(max_newton, int) or max_newton < 1:
        raise ValueError("max_newton must be a positive int, got %r" % (max_newton,))
    if w0 is not None and (not torch.is_tensor(w0) or w0.numel() != m or not w0.is_floating_point()):
        raise ValueError("w0 must be a float tensor of %d weights" % m)
    return n, m, s, mean


def spectral_laplace_fit(Z, y, observed=None, family="bernoulli", outputscale=1.0, exposure=None, trials=None, dispersion=None,
                         num_categories=None, cutpoints=None, mean=0.0, rtol=1e-10, max_newton=50, w0=None):
    """The mode of psi(w) (module docstring) by Newton's method in float64 with step halving: SpectralLaplaceFit.
    Z [n, m] float32: the training rows' features (kernel.features(train_x)), m <= 512; y [n]: labels, counts or categories, read
    at `observed` (bool [n]; None: every row; NaN allowed elsewhere); family: "bernoulli", "poisson" (exposure= [n]), "binomial"
    (trials= [n]), "negative_binomial" (dispersion=, exposure=) or "ordinal" (num_categories=, cutpoints= or None: the frequency
    logits of ordinal.ordinal_cutpoints), each checked with the rules and messages of its node fit; outputscale: s of
    K = s Z Z^T; mean: the constant prior mean of the latent function.  Stops when max |grad| <= rtol times its value at w = 0;
    one host read per evaluation; a step is halved at most MAX_HALVINGS times.  w0 [m]: the start (default 0)."""
    rec = families._family(family, "spectral")
    n, m, s, mean = _check_fit_args(Z, outputscale, mean, rtol, max_newton, w0)
    r = cuts = None
    if rec.data != "categories" and (num_categories is not None or cutpoints is not None):
        raise ValueError("num_categories and cutpoints belong to the ordinal family")
    if rec.data != "counts" and (exposure is not None or trials is not None or dispersion is not None):
        raise ValueError("exposure, trials and dispersion belong to the count families")
    if rec.data == "labels":
        y, observed = families.check_labels(y, observed, n)
        a64, b64, const = torch.nan_to_num(y.reshape(-1).double(), nan=0.0), None, None
    elif rec.data == "categories":
        if num_categories is None:
            raise ValueError("family %r needs %s" % (family, rec.needs))
        labels, observed, cuts = _check_categories(n, y, num_categories, cutpoints, observed)
        inf = torch.full((1,), float("inf"), dtype=torch.float64)
        a64 = torch.cat([-inf, cuts])[labels.cpu()]
        b64 = torch.cat([cuts, inf])[labels.cpu()]
        const = rec.constant(labels.cpu(), None, cuts)
    else:
        r = families.check_dispersion(rec, dispersion)
        y, observed, extra = families.check_counts(rec, n, y, observed, exposure, trials)
        seen = torch.ones(n, dtype=torch.bool, device=y.device) if observed is None else observed
        a64 = torch.where(seen, y, torch.zeros_like(y))
        if extra is None:
            b64 = None
        else:
            extra = torch.where(seen.to(extra.device), extra, torch.ones_like(extra))
            b64 = extra.log() if rec.aux != "trials" else extra
        const = rec.constant(a64, None if rec.aux != "trials" else b64.to(a64.device), r)
    _lib.require_device(Z, y, observed, exposure, trials, w0)
    dev = Z.device
    Z = _lib.f32c(Z)
    obs = None if observed is None else observed.to(dev).contiguous()
    a32 = a64.to(dev).float().contiguous()
    b32 = None if b64 is None else b64.to(dev).float().contiguous()
    if const is None:
        const = 0.0
    else:
        const = const.to(dev)
        const = float((const if obs is None else const[obs]).sum())

    def evaluate(w, hessian):
        f, grad, hess, sums = spectral_site(Z, w, family, a32, b32, obs, mean, r, hessian)
        g = grad - w / s
        ll, fmax, ww, gmax = torch.stack([sums[0], sums[1], w.dot(w), g.abs().max()]).tolist()   # the one host read
        return dict(w=w, f=f, g=g, hess=hess, ll=ll, fmax=fmax, quad=0.5 * ww / s, gmax=gmax, psi=ll - 0.5 * ww / s)

    with torch.no_grad():
        zero = torch.zeros(m, dtype=torch.float64, device=dev)
        if w0 is None:
            cur = evaluate(zero, True)
            grad0 = cur["gmax"]
        else:
            grad0 = evaluate(zero, False)["gmax"]
            cur = evaluate(w0.to(dev).reshape(-1).to(torch.float64), True)
        eye = torch.eye(m, dtype=torch.float64, device=dev) / s
        history, converged, its = [], False, 0
        while True:
            if not all(math.isfinite(cur[k]) for k in ("ll", "fmax", "quad", "gmax")):
                raise RuntimeError("spectral_laplace_fit: the latent values are not finite")
            if cur["gmax"] <= rtol * grad0:
                converged = True
                break
            if its >= max_newton:
                break
            chol = torch.linalg.cholesky(cur["hess"] + eye)
            delta = torch.cholesky_solve(cur["g"][:, None], chol)[:, 0]
            step, trial = 1.0, None
            for k in range(MAX_HALVINGS + 1):
                t = evaluate(cur["w"] + step * delta, k == 0)       # the full step is taken as a rule: its Hessian comes along
                slack = SLACK * max(abs(cur["ll"]) + cur["quad"], abs(t["ll"]) + t["quad"])
                if t["psi"] >= cur["psi"] - slack:
                    trial = t
                    break
                step *= 0.5
            if trial is None:
                warnings.warn("spectral_laplace_fit: no ascent after %d halvings of the Newton step (relative gradient %.3g)"
                              % (MAX_HALVINGS, cur["gmax"] / grad0))
                break
            cur = trial
            its += 1
            history.append((cur["psi"], cur["gmax"] / grad0, step))
            if cur["hess"] is None:
                cur = evaluate(cur["w"], True)
        if not converged and its >= max_newton:
            warnings.warn("spectral_laplace_fit: not converged in %d Newton steps (relative gradient %.3g)"
                          % (its, cur["gmax"] / grad0))
        chol = torch.linalg.cholesky(cur["hess"] + eye)
    return SpectralLaplaceFit(cur["w"], chol, cur["f"] + mean, converged, its, history, cur["ll"] + const, family, s, mean, r,
                              None if cuts is None else cuts.to(dev))
