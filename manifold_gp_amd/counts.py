"""Count data at the graph nodes: the Laplace approximation of a graph Matern GP with a Poisson, a binomial or a negative-binomial
likelihood (docs/kernels/counts.md).

With Q2 the form-0 precision of sampling.py, f the latent function and eta_i = f_i + mean (+ log E_i) the linear predictor,

    poisson:   y_i ~ Poisson(E_i exp(eta_i))            l = y eta - mu,                    g = y - mu,               h = mu
    binomial:  y_i ~ Binomial(N_i, sigma(eta_i))        l = y log pi + (N - y) log(1 - pi),  g = y (1 - pi) - (N - y) pi,  h = N pi (1 - pi)
    negative_binomial:  y_i ~ NB(mean mu_i = E_i exp(eta_i), dispersion r), Var y = mu + mu^2 / r: with pi = mu / (r + mu)
                                                        l = y log pi + r log(1 - pi),      g = y (1 - pi) - r pi,    h = (y + r) pi (1 - pi)

at the observed nodes (g = h = 0 elsewhere), the mode of psi(f) = sum_obs l_i - 1/2 f^T Q2 f is found by the Newton loop of
classification.py (_newton): a step solves (H + Q2) delta = g - Q2 f, which multiplied by s_ref is operator form 3 with
obs_w = s_ref h and noise = s_ref.  The per-node stage is one kernel (mgp_count_site); Q2 f comes from the float64 chain
(classification._q2); the solve is the library's Jacobi-preconditioned CG.

s_ref is a power of two fixed once per fit from the data, so one CG plan serves every step and (float)(s_ref h) is the scaled
correctly rounded h: 2^-ceil(log2 max(1, max y)) for Poisson (h = mu is about y at the mode; at a trial point w may exceed
1, which nothing in form 3 depends on: the operator, its Jacobi diagonal and the CG take any w >= 0) and 4 * 2^-ceil(log2 max N)
for the binomial (h <= N / 4, so w <= 1; at N = 1 this is the Bernoulli fit's 4), and 4 * 2^-ceil(log2 ceil(max y + r)) for the
negative binomial (h <= (y + r) / 4).  Its dispersion r is one scalar per fit: dispersion_profile fits a list of candidates and
compares their Laplace evidence; evidence.laplace_evidence(dispersion=) carries d log Z / dr (three sums over the nodes,
mgp_nb_dispersion_sums / nb_dispersion_sums), DispersionParameter states r = exp(rho) and learn_dispersion runs Adam on it with
the kernel fixed; utils.laplace_train takes a DispersionParameter in fit_kw and trains it with the kernel.

The iteration stops by the size of an accepted full Newton step (step_tol), not by the gradient relative to max |g(0)|:
for counts max |g(0)| is the size of the largest count, and a gradient rule relative to it stops hundreds of times further
from the mode than the same rule does for 0/1 labels (docs/kernels/counts.md has the numbers).

The Laplace posterior N(f_hat, (Q2 + H)^-1) is the form-3 GMRF posterior with pseudo-noise 1 / h and pseudo-targets
f_hat + g / h: CountLaplaceFit supplies the family's (g, h) (families.TABLE) and inherits _pseudo, latent_variance / latent_samples.

The predictive distribution of a new count -- its pmf, the log density of held-out counts, exceedance probabilities and
equal-tailed intervals (CountLaplaceFit.predict_pmf / predict_log_density / predict_exceedance / predict_interval) -- comes from
one quadrature per (node, count) in float64 (mgp_count_predict_pmf / mgp_count_predict_logpmf, docs/kernels/count_predict.md).
"""
import math

import torch

from . import _lib, _sites, families, sampling
from ._lib import check, lib, ptr, stream
from .classification import H_FLOOR, LaplaceFit, _newton_form3, _points
from ._sites import _int, _node_vector, _real
from .families import DISPERSION_MAX, DISPERSION_MIN, ETA_MAX, MAX_COUNT, check_dispersion, nb_log_constant  # noqa: F401

FAMILIES = families.codes("count")
_NB = families.TABLE[families.with_own("nb")]        # the family with entry points of its own (mgp_nb_*)
NB = _NB.count               # mgp_count_* refuse every code but the other two
PMF_POINTS = 65              # the default rule of the predictive pmf (docs/kernels/count_predict.md)
PMF_MAX_BLOCK = 65536        # counts per node in one mgp_count_predict_pmf call


def _count_family(family, dispersion, aux):
    """(record, dispersion as check_dispersion returns it) of a count family; aux: what a kernel wrapper got, which has to hold
    the trials of the binomial family"""
    rec = families._family(family, "count")
    r = check_dispersion(rec, dispersion)
    if rec.aux == "trials" and aux is None:
        raise ValueError("the binomial family needs the trials in aux")
    return rec, r


def count_site(f, qf, y, aux, observed, s_ref, mean, family, dispersion=None):
    """(w, rhs, sums) of mgp_count_site (mgp_nb_site for family "negative_binomial", with its dispersion): w = s_ref h and rhs = s_ref (g - qf) as fresh float32 [n] tensors (saturated at
    +-FLT_MAX), sums [4] float64 on the device (sum_obs l without the f-independent constant, sum f qf, max |g - qf|,
    sum (g - qf)^2).  f, y [n] float32; qf [n] or None (zeros); aux [n]: the log-exposure (family "poisson"; None: zeros) or the
    trials (family "binomial"); observed [n] bool or None (every node); mean: the constant added to f in the linear predictor."""
    rec, r = _count_family(family, dispersion, aux)
    site, name, workspace_bytes, code = families.stage(rec, "site", r)
    f, qf, (y, aux), observed, n, w, rhs, sums, work = _sites.newton_args(
        f, qf, (("y", y),), (("aux", aux),), observed, "count_site", workspace_bytes)
    check(site(ptr(f), ptr(qf), ptr(y), ptr(aux), ptr(observed), n, float(s_ref), float(mean), code, ptr(w), ptr(rhs), ptr(sums),
               ptr(work), work.numel(), stream()), name)
    return w, rhs, sums


def nb_dispersion_sums(f, y, aux, observed, variance, u, mean, dispersion, h_floor=H_FLOOR):
    """The three rows of d log Z / dr of a negative-binomial fit, r its dispersion (mgp_nb_dispersion_sums): [3] float64 on the
    device -- the likelihood's term with d c(y, r) / dr, the curvature's at fixed f (0 when variance is None) and the one through
    the mode (0 when u is None); their sum is the derivative, the mean and the exposure held fixed.  f [n] float32: the mode;
    y [n] the counts and aux [n] the log-exposure (None: zeros), read at observed nodes only; observed [n] bool or None;
    variance [n]: diag(A^-1) and u [n]: A^-1 (variance o h'), taken as float64; mean: the constant of the linear predictor."""
    r = check_dispersion(_NB, dispersion)
    n = _sites.check_evidence_args(f, (("y", y),), (("aux", aux),), observed, variance, h_floor, (("u", u),))
    _lib.require_device(f, y, aux, observed, variance, u)
    f, y = _lib.f32c(f.reshape(-1)), _lib.f32c(y.reshape(-1))
    aux = None if aux is None else _lib.f32c(aux.reshape(-1))
    observed = None if observed is None else observed.reshape(-1).contiguous()
    variance = None if variance is None else variance.reshape(-1).to(torch.float64).contiguous()
    u = None if u is None else u.reshape(-1).to(torch.float64).contiguous()
    out = torch.empty(3, dtype=torch.float64, device=f.device)
    work = _lib.workspace(lib().mgp_nb_dispersion_sums_workspace_bytes(n), "evidence_site", f.device)
    check(lib().mgp_nb_dispersion_sums(ptr(f), ptr(y), ptr(aux), ptr(observed), ptr(variance), ptr(u), n, float(mean), r,
                                       float(h_floor), ptr(out), ptr(work), work.numel(), stream()), "mgp_nb_dispersion_sums")
    return out


def _pmf_points(points):
    if isinstance(points, bool) or not isinstance(points, int) or not 17 <= points <= 257 or points % 2 == 0:
        raise ValueError("points must be an odd int in 17 .. 257, got %r" % (points,))
    return points


def _count_range(kmin, kmax):
    kmin, kmax = _int(kmin, "kmin"), _int(kmax, "kmax")
    if not 0 <= kmin <= kmax <= MAX_COUNT or kmax - kmin + 1 > PMF_MAX_BLOCK:
        raise ValueError("counts kmin .. kmax must lie in [0, 2^24] and number at most %d, got %d .. %d" % (PMF_MAX_BLOCK, kmin, kmax))
    return kmin, kmax


def _predict_inputs(eta, var, aux, family, dispersion=None):
    """(family record, eta, var as contiguous float64 [n], aux as contiguous float32 [n] or None, the dispersion or None), on the
    device"""
    rec, r = _count_family(family, dispersion, aux)
    _lib.require_device(eta, var, aux)
    eta = eta.reshape(-1).to(torch.float64).contiguous()
    var = var.reshape(-1).to(torch.float64).contiguous()
    aux = None if aux is None else _lib.f32c(aux.reshape(-1))
    for name, t in (("var", var), ("aux", aux)):
        if t is not None and t.shape[0] != eta.shape[0]:
            raise ValueError("%s has %d entries, eta %d" % (name, t.shape[0], eta.shape[0]))
    return rec, eta, var, aux, r


def count_predict_pmf(eta, var, aux, family, kmin, kmax, points=PMF_POINTS, log=False, dispersion=None):
    """The predictive pmf of the counts kmin .. kmax at every node: [n, kmax - kmin + 1] float64 (mgp_count_predict_pmf), its
    log with log=True.  eta [n]: the linear predictor at the mode without the exposure, var [n]: the latent marginal variance
    (both taken as float64; var <= 2^-76, negative entries included: the plain pmf at eta); aux [n] as count_site takes it:
    the log-exposure (family "poisson" and "negative_binomial", the latter with its dispersion, mgp_nb_predict_pmf; None: zeros)
    or the trials (family "binomial").  At most 65536 counts per call."""
    points = _pmf_points(points)
    kmin, kmax = _count_range(kmin, kmax)
    rec, eta, var, aux, r = _predict_inputs(eta, var, aux, family, dispersion)
    n, K = eta.shape[0], kmax - kmin + 1
    out = torch.empty((n, K), dtype=torch.float64, device=eta.device)
    pmf, name, _, code = families.stage(rec, "predict_pmf", r)
    check(pmf(ptr(eta), ptr(var), ptr(aux), n, code, kmin, K, points, int(bool(log)), ptr(out), stream()), name)
    return out


def count_predict_logpmf(eta, var, aux, y, at, family, points=PMF_POINTS, dispersion=None):
    """The log predictive probability of the one count y_i per node: [n] float64 (mgp_count_predict_logpmf), NaN outside the
    bool mask at [n] (None: every node).  y [n] integers in [0, 2^24] (taken as float32; not read outside at, NaN allowed
    there); eta, var, aux, dispersion as count_predict_pmf."""
    points = _pmf_points(points)
    if at is not None and (not torch.is_tensor(at) or at.dtype != torch.bool):
        raise ValueError("at must be a bool tensor [n]")
    rec, eta, var, aux, r = _predict_inputs(eta, var, aux, family, dispersion)
    _lib.require_device(y, at)
    n = eta.shape[0]
    y = _lib.f32c(y.reshape(-1))
    at = None if at is None else at.reshape(-1).contiguous()
    for name, t in (("y", y), ("at", at)):
        if t is not None and t.shape[0] != n:
            raise ValueError("%s has %d entries, eta %d" % (name, t.shape[0], n))
    out = torch.empty(n, dtype=torch.float64, device=eta.device)
    logpmf, name, _, code = families.stage(rec, "predict_logpmf", r)
    check(logpmf(ptr(eta), ptr(var), ptr(aux), ptr(y), ptr(at), n, code, points, ptr(out), stream()), name)
    return out


def _ceil_log2(m):
    """ceil(log2 m) of an integer m >= 1, exactly"""
    return (int(m) - 1).bit_length()


def _validate(desc, y, observed, family, exposure, trials, mean, step_tol, f0, dispersion=None):
    """The host-side argument checks of laplace_fit_counts / laplace_fit_negative_binomial, before any device call.  Returns
    (y, observed, extra, mean, s_ref) with y and extra (exposure or trials; None: ones) float64 [n] on the device they came on.
    dispersion: the negative binomial's, already checked (families.check_dispersion); it enters s_ref."""
    sampling._check_desc(desc)
    rec = families._family(family, "count")
    n = desc.n
    y, observed, extra = families.check_counts(rec, n, y, observed, exposure, trials)
    pick = _sites.picker(observed)
    seen = pick(y)
    if mean is not None:
        mean = _real(mean, "mean")
        if not math.isfinite(mean):
            raise ValueError("mean must be finite, got %r" % (mean,))
    if not _real(step_tol, "step_tol") > 0.0:
        raise ValueError("step_tol must be positive, got %r" % (step_tol,))
    if f0 is not None and (not torch.is_tensor(f0) or f0.numel() != n):
        raise ValueError("f0 must be a tensor of %d latent values" % n)
    if rec.aux != "trials":
        total = float(seen.sum())
        if mean is None:
            if total == 0.0:
                raise ValueError("every observed count is 0: the intercept-only estimate of the mean is -inf; pass mean=")
            mean = math.log(total / (float(seen.numel()) if extra is None else float(pick(extra).sum())))
        if rec.extra is None:
            s_ref = 2.0 ** -_ceil_log2(max(1.0, float(seen.max())))
        else:                                             # h <= (y + r) / 4: w <= 1 as for the binomial
            s_ref = 4.0 * 2.0 ** -_ceil_log2(math.ceil(float(seen.max()) + dispersion))
    else:
        mean = 0.0 if mean is None else mean
        s_ref = 4.0 * 2.0 ** -_ceil_log2(float(pick(extra).max()))
    return y, observed, extra, float(mean), s_ref


class CountLaplaceFit(LaplaceFit):
    """The Laplace approximation N(mean, (Q2 + H)^-1) of the latent posterior given counts (laplace_fit_counts).
    mean [n] float32: the mode f_hat of the latent function (the linear predictor is eta_hat = f_hat + prior_mean, plus the
    log-exposure inside the Poisson rate); converged, iterations; history: one (psi, relative gradient, step, CG iterations)
    per Newton step, psi without the likelihood's constant; log_likelihood: sum_obs log p(y_i | eta_hat_i) with the constant
    (-lgamma(y + 1), log C(N, y) or lgamma(y + r) - lgamma(r) - lgamma(y + 1)); family, prior_mean, s_ref; dispersion: r of the
    negative binomial, None otherwise; exposure / trials: float64 [n], 1 where none was given (prediction at unobserved nodes
    is per unit exposure / per trial there)."""

    def __init__(self, desc, y, observed, mean, converged, iterations, history, log_likelihood, family, prior_mean, s_ref,
                 aux, extra, dispersion=None):
        super().__init__(desc, y, observed, mean, converged, iterations, history, log_likelihood)
        self.family, self.prior_mean, self.s_ref, self.dispersion = family, prior_mean, s_ref, dispersion
        self._aux = aux                       # what the kernel read: float32 log-exposure (or None) / float32 trials
        if family != "binomial":
            self.exposure, self.trials = extra, None
        else:
            self.exposure, self.trials = None, extra

    def eta(self):
        """f_hat + prior_mean: the linear predictor at the mode without the exposure, float64 [n]."""
        return self.mean.double() + self.prior_mean

    def _gh(self, f, obs):
        y = torch.where(obs, self.y.double(), torch.zeros_like(f))
        rec = families.TABLE[self.family]
        if rec.aux == "trials":
            return rec.gh(self.eta(), y, self._aux.double(), None)
        # (_aux is finite at every node: laplace_fit_counts)
        return rec.gh(self.eta() if self._aux is None else self.eta() + self._aux.double(), y, None, self.dispersion)

    def _weights(self):
        return count_site(self.mean, None, self.y, self._aux, self.observed, self.s_ref, self.prior_mean, self.family,
                          self.dispersion)[0]

    def map_proba(self):
        raise NotImplementedError("a count fit has no class probability: see map_mean and predict_mean")

    def predict_proba(self, *a, **kw):
        raise NotImplementedError("a count fit has no class probability: see map_mean and predict_mean")

    def map_mean(self):
        """E exp(eta_hat) (Poisson, negative binomial) or N sigma(eta_hat) (binomial): the expected count at the mode, [n] float64
        (ignores the latent variance)."""
        if self.family != "binomial":
            return self.exposure * torch.exp(self.eta())
        return self.trials * torch.sigmoid(self.eta())

    def predict_mean(self, S=64, seed=None, points=129):
        """(mean, var, latent_var): the mean and the variance of a new count at every node under the Laplace posterior, and the
        latent marginal variance v they used (latent_variance(S, seed)[0]); float64 [n] each.  The formulas are
        families.count_moments': closed forms for the Poisson and the negative binomial, a quadrature for the binomial."""
        points = _points(points)
        v = self.latent_variance(S, seed)[0]
        return self._moments(v, points) + (v,)

    def _moments(self, v, points=129):
        extra = self.exposure if self.trials is None else self.trials
        return families.count_moments(families.TABLE[self.family], self.eta(), v, extra, self.dispersion, points)

    # -------------------------------------------------------------------------- the predictive distribution of a new count
    def _variance(self, variance, S, seed):
        """the latent marginal variance a predict_* call uses: the caller's (a latent_variance result) or latent_variance(S, seed)[0]"""
        if variance is None:
            return self.latent_variance(S, seed)[0]
        n = self.mean.shape[0]
        if not torch.is_tensor(variance) or variance.numel() != n or variance.dtype == torch.bool:
            raise ValueError("variance must be a tensor of %d latent marginal variances" % n)
        _lib.require_device(variance)
        return variance.reshape(-1).to(torch.float64)

    def _predict_args(self):
        """(eta, aux) of the predict kernels.  Poisson and negative binomial: the log-exposure is added to eta in float64 and aux is None -- the
        kernel's float32 log-exposure would cost 1e-7 of the rate, and the pmf would miss predict_mean's mean by as much.
        Binomial: eta and the trials as float32 (integers: exact)."""
        if self.family != "binomial":
            return self.eta() + self.exposure.log(), None
        return self.eta(), self.trials.float()

    def predict_pmf(self, kmax, S=64, seed=None, points=PMF_POINTS, kmin=0, variance=None, log=False):
        """(pmf, latent_var): P(y_new = k) for k = kmin .. kmax at every node under the Laplace posterior, [n, kmax - kmin + 1]
        float64 (its log with log=True), and the latent marginal variance it used [n]: `variance` (a latent_variance result) or
        latent_variance(S, seed)[0] as predict_mean.  Exposure and trials are the fit's own, 1 where none was given at an
        unobserved node.  A quadrature of its own per (node, k) with `points` nodes (docs/kernels/count_predict.md)."""
        points = _pmf_points(points)
        kmin, kmax = _count_range(kmin, kmax)
        v = self._variance(variance, S, seed)
        eta, aux = self._predict_args()
        return count_predict_pmf(eta, v, aux, self.family, kmin, kmax, points, log, self.dispersion), v

    def predict_log_density(self, y, at=None, S=64, seed=None, points=PMF_POINTS, variance=None):
        """log P(y_new = y_i) at the nodes of the bool mask at [n] (None: every node) under the Laplace posterior, float64 [n], NaN
        elsewhere: the log predictive density of held-out counts.  y [n]: integers in [0, 2^24] at those nodes, at most the fit's
        trials there for the binomial family; not read elsewhere (NaN allowed)."""
        points = _pmf_points(points)
        n = self.mean.shape[0]
        y = _node_vector(y, n, "y")
        if at is not None:
            if not torch.is_tensor(at) or at.dtype != torch.bool or at.dim() != 1 or at.shape[0] != n:
                raise ValueError("at must be a bool tensor [%d]" % n)
            if not bool(at.any()):
                raise ValueError("at selects no node")
        pick = (lambda t: t) if at is None else (lambda t: t[at.to(t.device)])
        asked = pick(y)
        if not bool(((asked >= 0) & (asked <= MAX_COUNT) & (asked == asked.round())).all()):
            raise ValueError("counts at the nodes asked for must all be integers in [0, 2^24]")
        if self.family == "binomial" and not bool((asked.to(self.trials.device) <= pick(self.trials)).all()):
            raise ValueError("counts must be at most the fit's trials at the nodes asked for")
        v = self._variance(variance, S, seed)
        _lib.require_device(y, at)
        eta, aux = self._predict_args()
        return count_predict_logpmf(eta, v, aux, y, at, self.family, points, self.dispersion)

    def predict_exceedance(self, threshold, S=64, seed=None, points=PMF_POINTS, variance=None):
        """P(y_new > threshold) at every node, float64 [n]: 1 - sum_{k <= threshold} pmf(k) on the pmf block 0 .. max threshold
        (clamped at 0).  threshold: an int or an integer tensor [n], 0 .. 65535 (one block of predict_pmf)."""
        points = _pmf_points(points)
        n = self.mean.shape[0]
        thr, top = _sites.threshold(threshold, n, "threshold", PMF_MAX_BLOCK - 1)
        pmf, _ = self.predict_pmf(top, S, seed, points, variance=variance)
        if thr is not None:
            keep = torch.arange(top + 1, device=pmf.device)[None, :] <= thr.to(pmf.device)[:, None]
            pmf = torch.where(keep, pmf, torch.zeros((), dtype=pmf.dtype, device=pmf.device))
        return (1.0 - pmf.sum(1)).clamp_min(0.0)

    def predict_interval(self, level=0.9, kmax=None, S=64, seed=None, points=PMF_POINTS, variance=None):
        """(lo, hi, reached): the equal-tailed predictive interval of a new count at every node -- the quantiles (1 - level) / 2
        and (1 + level) / 2 of the predictive cdf (the least k whose cdf is at least the level), int64 [n] -- from cumulative sums
        of the pmf block 0 .. kmax.  reached [n] bool: False where the upper quantile lies beyond kmax; hi = -1 there (and lo = -1
        where the lower one does).  kmax defaults to the largest predict_mean mean plus 8 of its standard deviations (Poisson,
        negative binomial) or the largest number of trials (binomial), capped at 65535."""
        points = _pmf_points(points)
        level = _real(level, "level")
        if not 0.0 < level < 1.0:
            raise ValueError("level must lie in (0, 1), got %r" % (level,))
        if kmax is not None:
            _, kmax = _count_range(0, kmax)
        v = self._variance(variance, S, seed)
        if kmax is None:
            if self.family != "binomial":
                m, var = self._moments(v)
                top = float((m + 8.0 * var.sqrt()).max())
            else:
                top = float(self.trials.max())
            kmax = int(min(math.ceil(top), PMF_MAX_BLOCK - 1)) if math.isfinite(top) else PMF_MAX_BLOCK - 1
        pmf, _ = self.predict_pmf(kmax, points=points, variance=v)
        cdf = pmf.cumsum(1)
        lo = (cdf < (1.0 - level) / 2.0).sum(1)
        hi = (cdf < (1.0 + level) / 2.0).sum(1)
        reached = hi <= kmax
        gone = torch.full_like(hi, -1)
        return torch.where(lo <= kmax, lo, gone), torch.where(reached, hi, gone), reached


def laplace_fit_counts(desc, y, observed=None, family="poisson", exposure=None, trials=None, mean=None, step_tol=1e-3,
                       max_newton=30, cg_tol=1e-3, max_iter=5000, f0=None):
    """The mode of the latent posterior given counts y [n] at the observed nodes (bool [n]; None: every node; counts at the
    other nodes are not read and may be NaN), by Newton's method with step halving: CountLaplaceFit.
    family "poisson": y_i ~ Poisson(exposure_i exp(f_i + mean)); exposure [n] finite and positive at the observed nodes (None:
    ones); mean: the constant prior mean of the linear predictor, default log(sum_obs y / sum_obs exposure), the
    intercept-only maximum-likelihood estimate.  family "binomial": y_i ~ Binomial(trials_i, sigma(f_i + mean)); trials [n]
    integers >= max(1, y_i) at the observed nodes; mean defaults to 0.  Counts and trials are integers up to 2^24.
    The negative binomial needs its dispersion and has a front of its own, laplace_fit_negative_binomial; fit_counts takes every
    family with dispersion=.
    Exposure / trials at unobserved nodes are used by predict_mean where they are valid and count as 1 elsewhere.
    desc: a form-0 precision descriptor as the samplers take.  Stops after an accepted full Newton step with
    max |delta| <= step_tol; every step is a form-3 CG solve to the relative residual cg_tol.  f0 [n]: the start (default 0)."""
    if families._family(family, "count").extra is not None:
        raise ValueError("the negative_binomial family needs dispersion=: laplace_fit_negative_binomial(desc, y, dispersion, ...) "
                         "or fit_counts(..., family=, dispersion=)")
    return _fit(desc, y, observed, family, exposure, trials, mean, step_tol, max_newton, cg_tol, max_iter, f0, None)


def laplace_fit_negative_binomial(desc, y, dispersion, observed=None, exposure=None, mean=None, step_tol=1e-3, max_newton=30,
                                  cg_tol=1e-3, max_iter=5000, f0=None):
    """Overdispersed counts: laplace_fit_counts with y_i ~ NB(mean exposure_i exp(f_i + mean), dispersion), variance
    mean + mean^2 / dispersion.  dispersion: one finite scalar in [2^-10, 2^20], fixed (the Poisson family is its limit
    dispersion -> inf, 1 is the geometric distribution; dispersion_profile compares candidates by their evidence); exposure, the
    default mean log(sum_obs y / sum_obs exposure) and every other argument as laplace_fit_counts takes them for Poisson."""
    return _fit(desc, y, observed, "negative_binomial", exposure, None, mean, step_tol, max_newton, cg_tol, max_iter, f0, dispersion)


def fit_counts(desc, y, observed=None, family="poisson", dispersion=None, **kw):
    """The count fit of any family: family "negative_binomial" with dispersion= (required there, refused elsewhere) goes to
    laplace_fit_negative_binomial, "poisson" and "binomial" to laplace_fit_counts; kw as those take them."""
    if check_dispersion(families._family(family, "count"), dispersion) is None:
        return laplace_fit_counts(desc, y, observed, family, **kw)
    if kw.get("trials") is not None:
        raise ValueError("trials belong to the binomial family; the Poisson and negative_binomial families take exposure")
    kw.pop("trials", None)
    return laplace_fit_negative_binomial(desc, y, dispersion, observed, **kw)


def _fit(desc, y, observed, family, exposure, trials, mean, step_tol, max_newton, cg_tol, max_iter, f0, dispersion):
    """laplace_fit_counts and laplace_fit_negative_binomial: the checks, the constant of the likelihood and the Newton loop"""
    rec = families._family(family, "count")
    r = check_dispersion(rec, dispersion)
    y, observed, extra, mean, s_ref = _validate(desc, y, observed, family, exposure, trials, mean, step_tol, f0, r)
    _lib.require_device(y, f0, extra)
    dev = desc.data.graph.device
    n = desc.n
    y = y.to(dev)
    obs = None if observed is None else observed.to(dev).contiguous()
    seen = torch.ones(n, dtype=torch.bool, device=dev) if obs is None else obs
    one, zero = torch.ones((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    y = torch.where(seen, y, zero)                        # (NaN at unobserved nodes: never read, dropped here)
    if extra is None:
        extra, aux = torch.ones(n, dtype=torch.float64, device=dev), None
    else:
        extra = extra.to(dev)
        valid = torch.isfinite(extra) & (extra > 0) if family != "binomial" else (extra >= 1) & (extra == extra.round())
        extra = torch.where(seen | valid, extra, one)
        aux = (extra.log() if family != "binomial" else extra).float().contiguous()
    const = float(rec.constant(y[seen], extra[seen], r).sum())
    y32 = y.float().contiguous()

    f, sums, converged, its, history = _newton_form3(
        "laplace_fit_counts", desc, lambda f, qf: count_site(f, qf, y32, aux, obs, s_ref, mean, family, r), s_ref, f0, 0.0,
        max_newton, cg_tol, max_iter, step_tol=float(step_tol))
    return CountLaplaceFit(desc, y32, obs, f, converged, its, history, sums[0] + const, family, mean, s_ref, aux, extra, r)


class DispersionParameter(torch.nn.Module):
    """The negative binomial's dispersion as a differentiable function of one unconstrained float64 parameter raw = rho = log r:
    forward() = exp(rho) with rho clamped to [log 2^-10, log 2^20], a 0-dim float64 tensor.  init: the start, a scalar in
    [2^-10, 2^20], which forward() returns exactly until raw moves (the exponential is taken of rho - log init)."""

    def __init__(self, init):
        super().__init__()
        r = check_dispersion(_NB, init)
        self.register_buffer("init", torch.tensor(r, dtype=torch.float64))
        self.register_buffer("rho0", torch.tensor(math.log(r), dtype=torch.float64))
        self.raw = torch.nn.Parameter(self.rho0.clone())

    def forward(self):
        lo, hi = math.log(DISPERSION_MIN), math.log(DISPERSION_MAX)
        r = (self.init * torch.exp(self.raw.clamp(lo, hi) - self.rho0)).clamp(DISPERSION_MIN, DISPERSION_MAX)
        bound = torch.full_like(r, DISPERSION_MAX).where(self.raw > hi, torch.full_like(r, DISPERSION_MIN))
        return torch.where((self.raw > hi) | (self.raw < lo), bound, r)                    # a clamped rho: the bound itself


def _live_dispersion(fit_kw):
    """(fit_kw with the dispersion as a float, the live tensor or None): a dispersion given as a DispersionParameter is evaluated
    now; a tensor that requires grad, its or the caller's, is what laplace_evidence differentiates.  Anything else passes as it
    is."""
    r = fit_kw.get("dispersion")
    if isinstance(r, torch.nn.Module):
        r = r()
        fit_kw = dict(fit_kw, dispersion=r.detach())
    if not torch.is_tensor(r) or not r.requires_grad:
        return fit_kw, None
    if r.numel() != 1:
        raise ValueError("dispersion must be a real scalar, got a tensor of shape %s" % (tuple(r.shape),))
    return dict(fit_kw, dispersion=float(r.detach())), r


def learn_dispersion(desc, y, dispersion0, observed=None, exposure=None, mean=None, steps=30, lr=0.1, var_samples=64, variance=None,
                     fit_kw=None, evidence_kw=None):
    """Learn the negative binomial's dispersion on the Laplace evidence with the kernel hyper-parameters fixed: Adam(lr) for
    `steps` steps on a DispersionParameter started at dispersion0, loss -log Z / m, every fit warm-started from the previous
    mode, the gradient that of evidence.laplace_evidence(dispersion=).  variance: None (every step draws
    fit.latent_variance(var_samples)[0]), or a callable fit -> diag(A^-1) [n].  fit_kw as laplace_fit_negative_binomial takes,
    evidence_kw as laplace_evidence.  Returns (r, the CountLaplaceFit at it, history: one (r, log Z, se) per step, taken before
    the step's update).  Warns when r ends on a bound of [2^-10, 2^20]: 2^20 is the Poisson limit, which the data may prefer."""
    import warnings
    from .evidence import laplace_evidence
    steps = _sites.learning_args(steps, lr, variance)
    fit_kw, evidence_kw = dict(fit_kw or {}), dict(evidence_kw or {})
    param = DispersionParameter(dispersion0)
    opt = torch.optim.Adam(param.parameters(), lr=float(lr))
    f0, history = fit_kw.pop("f0", None), []
    for _ in range(steps):
        opt.zero_grad()
        r = param()
        fit = laplace_fit_negative_binomial(desc, y, float(r.detach()), observed, exposure, mean, f0=f0, **fit_kw)
        f0 = fit.mean
        ev = laplace_evidence(fit, variance=None if variance is None else variance(fit), var_samples=var_samples, dispersion=r,
                              **evidence_kw)
        history.append((fit.dispersion, float(ev.value.detach()), ev.se))
        (-ev.value / ev.m).backward()
        opt.step()
    r = float(param().detach())
    if r in (DISPERSION_MIN, DISPERSION_MAX):
        warnings.warn("learn_dispersion ended on the bound r = %g%s" % (r, ": the Poisson limit" if r == DISPERSION_MAX else ""))
    return r, laplace_fit_negative_binomial(desc, y, r, observed, exposure, mean, f0=f0, **fit_kw), history


def dispersion_profile(desc, y, dispersions, observed=None, exposure=None, mean=None, **kw):
    """Negative-binomial fits over a list of candidate dispersions and their Laplace evidence: (results, best) with results the
    list of (r, CountLaplaceFit, LaplaceEvidence) in the order given and best the index of the largest evidence value.  Every fit
    starts from the mode of the one before it (f0=), and every evidence is taken with the same keyword arguments -- the same
    seed and probes, so that the Lanczos error of the log-determinant is common to the candidates (up to 512 effective nodes
    the log-determinant is exact).  kw: keyword arguments of laplace_fit_counts (step_tol, max_newton, cg_tol, max_iter, f0: the
    first start) and of evidence.laplace_evidence (the others).  Host code only."""
    from .evidence import laplace_evidence
    fit_names = ("step_tol", "max_newton", "cg_tol", "max_iter", "f0")
    fit_kw = {k: v for k, v in kw.items() if k in fit_names}
    ev_kw = {k: v for k, v in kw.items() if k not in fit_names}
    for bad in ("family", "dispersion", "trials", "operator"):
        if bad in ev_kw:
            raise ValueError("dispersion_profile takes no %s=" % bad)
    try:
        candidates = [check_dispersion(_NB, r) for r in dispersions]
    except TypeError:
        raise ValueError("dispersions must be a sequence of scalars")
    if not candidates:
        raise ValueError("dispersions is empty")
    results, f0 = [], fit_kw.pop("f0", None)
    for r in candidates:
        fit = laplace_fit_negative_binomial(desc, y, r, observed, exposure, mean, f0=f0, **fit_kw)
        results.append((r, fit, laplace_evidence(fit, **ev_kw)))
        f0 = fit.mean
    values = [float(e.value) for _, _, e in results]
    return results, max(range(len(values)), key=values.__getitem__)
