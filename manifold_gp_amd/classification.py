"""Node classification: the Laplace approximation of a graph Matern GP with a Bernoulli-logit likelihood
(docs/kernels/classification.md).

With Q2 the form-0 precision of sampling.py, labels t_i in {0, 1} at the observed nodes and p(t_i | f_i) = sigma((2 t_i - 1) f_i),
the mode of  psi(f) = sum_obs log p(t_i | f_i) - 1/2 f^T Q2 f  is found by Newton's method.  With g = d log p / d f = t - sigma(f)
and h = -d^2 log p / d f^2 = sigma(f) (1 - sigma(f)) (both 0 at unobserved nodes) a step solves

    (H + Q2) delta = g - Q2 f                  H = diag(h)

which, multiplied by s_ref = 4, is operator form 3 with obs_w = 4 h in [0, 1] and noise = 4 (the weights of a form-3 system
lie in [0, 1]: h <= 1/4).  The per-node stage -- w, the right-hand side, and the four sums the step control reads -- is one
kernel (mgp_bernoulli_site); Q2 f comes from the float64 chain (Descriptor.apply_f64, see _q2); the solve is the library's
Jacobi-preconditioned CG (cg_solve).  The Laplace posterior
N(f_hat, (Q2 + H)^-1) is the form-3 GMRF posterior with pseudo-noise 1 / h and pseudo-targets f_hat + g / h: variances and
samples are sampling.posterior_variance / posterior_samples, nothing else.  The predictive class probability integrates
the logistic against the latent marginal (mgp_bernoulli_predict).
"""
import math
import warnings

import torch

from . import _lib, sampling
from ._lib import check, lib, ptr, stream

S_REF = 4.0              # obs_w = S_REF h <= 1
LINKS = {"logit": 0}
MAX_HALVINGS = 10
H_FLOOR = 1e-30          # an observed node below it carries no information at float32 weight resolution (latent_* drop it)
# Step control compares psi = sums[0] - sums[1] / 2 of the trial with psi of the current point.  The sums are float64 from
# the float32 f (the iterate itself: exact) and the float32 qf, which is Q2 f formed in float64 (_q2) and rounded once:
# |delta qf_i| <= u |qf_i|, u = 2^-24, so f^T qf / 2 is off by at most u / 2 sum |f_i qf_i|.  The kernel leaves sum f_i qf_i,
# not the sum of the absolute terms; the two differ by a small factor on a Newton path (f^T Q2 f >= 0 term by term but for
# the nodes where f and Q2 f disagree in sign).  The slack takes SLACK_ULPS u on |sums[0]| + |sums[1]| / 2 = |psi| -- a
# factor 32 over the bound with the signed sum --, at the larger of the two points: a decrease below it is rounding, one
# above it halves the step.  Convergence is judged by the gradient, never by psi.
SLACK_ULPS = 16.0
_U32 = 2.0 ** -24


def _slack(sums):
    return SLACK_ULPS * _U32 * (abs(sums[0]) + 0.5 * abs(sums[1]))


def _psi(sums):
    return sums[0] - 0.5 * sums[1]


def _q2(desc, f):
    """Q2 f rounded to float32 from the float64 chain.  The float32 chain (desc.apply) rounds after every factor of
    (tau I + L_sym)^nu, and the smooth f of a posterior mode cancels against it: on the 1546-node dumbbell (k = 10, nu = 3) its
    error at the mode is 5e-6, the size of rtol max |g(0)|, and Newton stalls at a relative gradient of 1.5e-5 to 1.9e-5."""
    return desc.apply_f64(f.double()).float()


def bernoulli_site(f, qf, y, observed=None, s_ref=S_REF, link="logit"):
    """(w, rhs, sums) of mgp_bernoulli_site: w = s_ref h and rhs = s_ref (g - qf) as fresh float32 [n] tensors, sums [4]
    float64 on the device (sum_obs log p, sum f qf, max |g - qf|, sum (g - qf)^2).  f, y [n] float32; qf [n] float32 or None
    (zeros); observed [n] bool or None (every node)."""
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    _lib.require_device(f, qf, y, observed)
    f, y = _lib.f32c(f.reshape(-1)), _lib.f32c(y.reshape(-1))
    n = f.shape[0]
    qf = None if qf is None else _lib.f32c(qf.reshape(-1))
    if observed is not None:
        if observed.dtype != torch.bool:
            raise ValueError("observed must be a bool tensor [n]")
        observed = observed.reshape(-1).contiguous()
    for name, t in (("qf", qf), ("y", y), ("observed", observed)):
        if t is not None and t.shape[0] != n:
            raise ValueError("%s has %d entries, f %d" % (name, t.shape[0], n))
    w, rhs = torch.empty_like(f), torch.empty_like(f)
    sums = torch.empty(4, dtype=torch.float64, device=f.device)
    wb = lib().mgp_bernoulli_site_workspace_bytes(n)
    work = _lib.workspace(wb, "bernoulli_site", f.device)
    check(lib().mgp_bernoulli_site(ptr(f), ptr(qf), ptr(y), ptr(observed), n, float(s_ref), LINKS[link], ptr(w), ptr(rhs),
                                   ptr(sums), ptr(work), work.numel(), stream()), "mgp_bernoulli_site")
    return w, rhs, sums


def _points(points):
    if isinstance(points, bool) or not isinstance(points, int) or not 9 <= points <= 1025 or points % 2 == 0:
        raise ValueError("points must be an odd int in 9 .. 1025, got %r" % (points,))
    return points


def bernoulli_predict(mean, var, points=129):
    """int sigma(mean_i + sqrt(var_i) u) phi(u) du by the `points`-point trapezoid rule on [-8, 8]: [n] float64
    (mgp_bernoulli_predict).  mean [n] (taken as float32), var [n] (taken as float64; negative entries count as 0)."""
    points = _points(points)
    _lib.require_device(mean, var)
    mean = _lib.f32c(mean.reshape(-1))
    var = var.reshape(-1).to(torch.float64).contiguous()
    if var.shape[0] != mean.shape[0]:
        raise ValueError("var has %d entries, mean %d" % (var.shape[0], mean.shape[0]))
    prob = torch.empty_like(var)
    check(lib().mgp_bernoulli_predict(ptr(mean), ptr(var), mean.shape[0], points, ptr(prob), stream()), "mgp_bernoulli_predict")
    return prob


def _validate(desc, y, observed, link, f0):
    """The host-side argument checks of laplace_fit: (y [n], observed [n] bool or None), on whatever device they came."""
    sampling._check_desc(desc)
    n = desc.n
    if link not in LINKS:
        raise ValueError("link must be one of %s, got %r" % (sorted(LINKS), link))
    if not torch.is_tensor(y) or y.numel() != n:
        raise ValueError("y must be a tensor of %d labels, got %s" % (n, tuple(y.shape) if torch.is_tensor(y) else type(y)))
    y = y.reshape(-1)
    if observed is not None:
        if not torch.is_tensor(observed) or observed.dtype != torch.bool:
            raise ValueError("observed must be a bool tensor [n]")
        if observed.dim() != 1 or observed.shape[0] != n:
            raise ValueError("observed has shape %s, the graph %d nodes" % (tuple(observed.shape), n))
        if not bool(observed.any()):
            raise ValueError("observed selects no node")
        observed = observed.to(y.device)
    seen = y if observed is None else y[observed]
    if not bool(((seen == 0) | (seen == 1)).all()):
        raise ValueError("labels at the observed nodes must all be 0 or 1")
    if f0 is not None and (not torch.is_tensor(f0) or f0.numel() != n):
        raise ValueError("f0 must be a tensor of %d latent values" % n)
    return y, observed


class LaplaceFit:
    """The Laplace approximation N(mean, (Q2 + H)^-1) of the latent posterior (laplace_fit).
    mean [n] float32: the mode; converged, iterations; history: one (psi, relative gradient, step, CG iterations) per
    Newton step; log_likelihood: sum_obs log p(t_i | mean_i)."""

    def __init__(self, desc, y, observed, mean, converged, iterations, history, log_likelihood):
        self.desc, self.y, self.observed = desc, y, observed
        self.mean, self.converged, self.iterations = mean, converged, iterations
        self.history, self.log_likelihood = history, log_likelihood

    def map_proba(self):
        """sigma(mean): the class-1 probability at the mode, [n] float64 (ignores the latent variance)."""
        return torch.sigmoid(self.mean.double())

    def _pseudo(self):
        """(pseudo-targets f_hat + g / h, pseudo-noise 1 / h, obs_eff) in float64 from the mode; entries outside obs_eff are
        0 and 1."""
        f = self.mean.double()
        e = torch.exp(-f.abs())
        h = e / (1.0 + e) ** 2
        obs = torch.ones_like(f, dtype=torch.bool) if self.observed is None else self.observed
        eff = obs & (h >= H_FLOOR)
        if not bool(eff.any()):
            raise RuntimeError("no observed node has a curvature above %g: the latent values have run away" % H_FLOOR)
        t = (torch.nan_to_num(self.y.double(), nan=0.0) > 0.5).double()
        g = t - torch.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        one, zero = torch.ones((), dtype=f.dtype, device=f.device), torch.zeros((), dtype=f.dtype, device=f.device)
        noise = torch.where(eff, 1.0 / h.clamp_min(H_FLOOR), one)
        targets = torch.where(eff, f + g * noise, zero)
        return targets, noise, eff

    def latent_variance(self, S=64, seed=None, **kw):
        """(var, se): diag((Q2 + H)^-1) at every node and its standard error, float64 [n] each: sampling.posterior_variance
        with the per-node noise 1 / h on the observed nodes (kw: method, tol, refine, max_iter)."""
        _, noise, eff = self._pseudo()
        return sampling.posterior_variance(self.desc, noise, S, seed, observed=eff, **kw)

    def latent_samples(self, S, seed=None):
        """f ~ N(mean, (Q2 + H)^-1): [S, n] float32: sampling.posterior_samples on the pseudo-targets f_hat + g / h."""
        targets, noise, eff = self._pseudo()
        return sampling.posterior_samples(self.desc, targets, noise, S, seed, observed=eff)

    def predict_proba(self, S=64, seed=None, points=129):
        """(p, var): the class-1 probability int sigma(f) N(f; mean_i, var_i) df at every node and the latent marginal
        variance it used (latent_variance(S, seed)[0]), float64 [n] each."""
        points = _points(points)
        var = self.latent_variance(S, seed)[0]
        return bernoulli_predict(self.mean, var, points), var


def laplace_fit(desc, y, observed=None, link="logit", rtol=1e-5, max_newton=30, cg_tol=1e-3, max_iter=5000, f0=None):
    """The mode of the latent posterior given 0/1 labels y [n] at the observed nodes (bool [n]; None: every node; labels at
    the other nodes are not read and may be NaN), by Newton's method with step halving: LaplaceFit.
    desc: a form-0 precision descriptor as the samplers take.  Stops when max |g - Q2 f| <= rtol times its value at f = 0;
    every step is a form-3 CG solve to the relative residual cg_tol.  f0 [n]: the starting point (default 0)."""
    from .solvers import cg_solve
    y, observed = _validate(desc, y, observed, link, f0)
    _lib.require_device(y, f0)
    dev = desc.data.graph.device
    n = desc.n
    y = _lib.f32c(y.to(dev))
    obs = None if observed is None else observed.to(dev).contiguous()

    def site(f, qf):
        w, rhs, sums = bernoulli_site(f, qf, y, obs, S_REF, link)
        return w, rhs, sums.tolist()                      # the one host read of an evaluation

    with torch.no_grad():
        zero = torch.zeros(n, dtype=torch.float32, device=dev)
        if f0 is None:
            f = zero
            w, rhs, sums = site(f, None)                  # Q2 0 = 0: no apply at the start
            grad0 = sums[2]
        else:
            grad0 = site(zero, None)[2][2]
            f = _lib.f32c(f0.to(dev).reshape(-1))
            w, rhs, sums = site(f, _q2(desc, f))
        history, converged, its = [], False, 0
        while True:
            if not all(math.isfinite(v) for v in sums):
                raise RuntimeError("laplace_fit: the latent values are not finite")
            if sums[2] <= rtol * grad0:
                converged = True
                break
            if its >= max_newton:
                break
            # a fresh w every evaluation: the CG plan is rebound by the tensor's address (solvers._cached_plan)
            delta, cg_its, _ = cg_solve(desc.with_(form=3, noise=S_REF, obs_w=w), rhs, tol=cg_tol, stop_mode=1,
                                        jacobi=sampling.OBSERVED_JACOBI[0], max_iter=max_iter)
            step, trial = 1.0, None
            for _ in range(MAX_HALVINGS + 1):
                ft = f + step * delta
                wt, rhst, sumst = site(ft, _q2(desc, ft))
                if _psi(sumst) >= _psi(sums) - max(_slack(sums), _slack(sumst)):
                    trial = (ft, wt, rhst, sumst)
                    break
                step *= 0.5
            if trial is None:
                warnings.warn("laplace_fit: no ascent after %d halvings of the Newton step (relative gradient %.3g)"
                              % (MAX_HALVINGS, sums[2] / grad0))
                break
            f, w, rhs, sums = trial
            its += 1
            history.append((_psi(sums), sums[2] / grad0, step, int(cg_its)))
    if not converged and its >= max_newton:
        warnings.warn("laplace_fit: not converged in %d Newton steps (relative gradient %.3g)" % (its, sums[2] / grad0))
    return LaplaceFit(desc, y, obs, f, converged, its, history, sums[0])
