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

C classes (laplace_fit_multiclass): labels t_i in {0 .. C-1}, F [n, C] row-major, the C latent functions with independent priors
of the same precision Q2, p(t_i | F_i) = softmax(F_i)[t_i].  The softmax ties the classes together at every observed node:
with Pi = softmax(F) row by row and G = onehot(t) - Pi (both 0 at unobserved rows) a step solves

    (Q2 (x) I_C + H) Delta = G - Q2 F          (H X)_i = pi_i o x_i - pi_i (pi_i . x_i)

ONE SPD system of size n C, which neither the multi-column CG (one set of scalars per column) nor form 3 (one weight vector
for all columns) expresses: mgp_softmax_cg solves it with one alpha and one beta per step, mgp_softmax_site is the per-row
likelihood stage; mgp_softmax_cg_block solves S such systems with the same matrix at once (the samples of a fit, block=).  The Newton loop itself (_newton) is the binary fit's, stated once.  At the mode every row of F sums to 0
(the prior fixes the softmax gauge).  Samples are perturb-and-MAP on the coupled system (MulticlassLaplaceFit.latent_samples),
class probabilities the samples' mean softmax.
"""
import ctypes
import math
import warnings

import torch

from . import _lib, _sites, families, sampling
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
    f, qf, (y,), observed, n, w, rhs, sums, work = _sites.newton_args(
        f, qf, (("y", y),), (), observed, "bernoulli_site", lib().mgp_bernoulli_site_workspace_bytes)
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
    y, observed = families.check_labels(y, observed, n)
    if f0 is not None and (not torch.is_tensor(f0) or f0.numel() != n):
        raise ValueError("f0 must be a tensor of %d latent values" % n)
    return y, observed


class LaplaceFit:
    """The Laplace approximation N(mean, (Q2 + H)^-1) of the latent posterior (laplace_fit).
    mean [n] float32: the mode; converged, iterations; history: one (psi, relative gradient, step, CG iterations) per
    Newton step; log_likelihood: sum_obs log p(t_i | mean_i).  family: the fit's row of families.TABLE; prior_mean, _aux, s_ref and
    dispersion are what the site kernels of the family read beside y (evidence._site_of)."""
    family, prior_mean, _aux, s_ref, dispersion = "bernoulli", 0.0, None, S_REF, None

    def __init__(self, desc, y, observed, mean, converged, iterations, history, log_likelihood):
        self.desc, self.y, self.observed = desc, y, observed
        self.mean, self.converged, self.iterations = mean, converged, iterations
        self.history, self.log_likelihood = history, log_likelihood

    def map_proba(self):
        """sigma(mean): the class-1 probability at the mode, [n] float64 (ignores the latent variance)."""
        return torch.sigmoid(self.mean.double())

    def _gh(self, f, obs):
        """(g, h) of the family in float64 at the mode f; obs: the observed nodes, the others are not used"""
        return families.TABLE[self.family].gh(f, self.y, None, None)

    def _weights(self):
        """obs_w = (float)(s_ref h) of the fit's own form-3 system at the mode, from the kernel its Newton steps used"""
        return bernoulli_site(self.mean, None, self.y, self.observed, self.s_ref)[0]

    def _pseudo(self):
        """(pseudo-targets f_hat + g / h, pseudo-noise 1 / h, obs_eff) in float64 from the mode, with the family's g and h
        (_gh); entries outside obs_eff are 0 and 1."""
        f = self.mean.double()
        obs = torch.ones_like(f, dtype=torch.bool) if self.observed is None else self.observed
        g, h = self._gh(f, obs)
        eff = obs & (h >= H_FLOOR)
        if not bool(eff.any()):
            raise RuntimeError("no observed node has a curvature above %g: the latent values have run away" % H_FLOOR)
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

    def evidence(self, **kw):
        """The Laplace approximation of log p(y) at this mode, an evidence.LaplaceEvidence; kw as evidence.laplace_evidence
        (operator= for the hyper-parameter gradient, num_probes, steps, seed, method, ...)."""
        from .evidence import laplace_evidence
        return laplace_evidence(self, **kw)


def _newton(name, site, q2, solve, zero, f0, rtol, max_newton, step_tol=None):
    """Newton's method with step halving on psi, stated once for every fit.  site(f, qf) -> (aux, rhs, sums) with sums a list
    (the one host read of an evaluation); q2(f) = Q2 f as float32; solve(aux, rhs) -> (delta, CG iterations); zero: the point
    f = 0; f0: the start (None: zero, where Q2 0 = 0 needs no apply).  Stops when sums[2] <= rtol times its value at f = 0;
    a trial point is taken when psi does not decrease beyond _slack, after at most MAX_HALVINGS halvings.
    step_tol (None: off, the classification fits): an accepted full step with max |delta| <= step_tol ends the iteration as
    converged too -- the Newton step is the distance to the mode up to its square (counts.py); one more host read per step.
    Returns (f, aux, sums, converged, steps, history)."""
    if f0 is None:
        f = zero
        aux, rhs, sums = site(f, None)
        grad0 = sums[2]
    else:
        grad0 = site(zero, None)[2][2]
        f = f0
        aux, rhs, sums = site(f, q2(f))
    history, converged, its = [], False, 0
    while True:
        if not all(math.isfinite(v) for v in sums):
            raise RuntimeError("%s: the latent values are not finite" % name)
        if sums[2] <= rtol * grad0:
            converged = True
            break
        if its >= max_newton:
            break
        delta, cg_its = solve(aux, rhs)
        step, trial = 1.0, None
        for _ in range(MAX_HALVINGS + 1):
            ft = f + step * delta
            auxt, rhst, sumst = site(ft, q2(ft))
            if _psi(sumst) >= _psi(sums) - max(_slack(sums), _slack(sumst)):
                trial = (ft, auxt, rhst, sumst)
                break
            step *= 0.5
        if trial is None:
            warnings.warn("%s: no ascent after %d halvings of the Newton step (relative gradient %.3g)"
                          % (name, MAX_HALVINGS, sums[2] / grad0))
            break
        f, aux, rhs, sums = trial
        its += 1
        history.append((_psi(sums), sums[2] / grad0, step, int(cg_its)))
        if step_tol is not None and step == 1.0 and float(abs(delta).max()) <= step_tol:
            converged = True
            break
    if not converged and its >= max_newton:
        warnings.warn("%s: not converged in %d Newton steps (relative gradient %.3g)" % (name, its, sums[2] / grad0))
    return f, aux, sums, converged, its, history


def laplace_fit(desc, y, observed=None, link="logit", rtol=1e-5, max_newton=30, cg_tol=1e-3, max_iter=5000, f0=None):
    """The mode of the latent posterior given 0/1 labels y [n] at the observed nodes (bool [n]; None: every node; labels at
    the other nodes are not read and may be NaN), by Newton's method with step halving: LaplaceFit.
    desc: a form-0 precision descriptor as the samplers take.  Stops when max |g - Q2 f| <= rtol times its value at f = 0;
    every step is a form-3 CG solve to the relative residual cg_tol.  f0 [n]: the starting point (default 0)."""
    y, observed = _validate(desc, y, observed, link, f0)
    _lib.require_device(y, f0)
    dev = desc.data.graph.device
    y = _lib.f32c(y.to(dev))
    obs = None if observed is None else observed.to(dev).contiguous()
    f, sums, converged, its, history = _newton_form3("laplace_fit", desc, lambda f, qf: bernoulli_site(f, qf, y, obs, S_REF, link),
                                                     S_REF, f0, rtol, max_newton, cg_tol, max_iter)
    return LaplaceFit(desc, y, obs, f, converged, its, history, sums[0])


def _newton_form3(name, desc, site, s_ref, f0, rtol, max_newton, cg_tol, max_iter, step_tol=None):
    """_newton for one latent function on the nodes (the binary, count and ordinal fits): site(f, qf) is the family's kernel,
    (w, rhs, sums on the device); a step is the form-3 CG solve with obs_w = w and noise = s_ref to the relative residual cg_tol.
    Returns (f, sums, converged, steps, history)."""
    from .solvers import cg_solve
    dev = desc.data.graph.device

    def evaluate(f, qf):
        w, rhs, sums = site(f, qf)
        return w, rhs, sums.tolist()                      # the one host read of an evaluation

    def solve(w, rhs):
        # a fresh w every evaluation: the CG plan is rebound by the tensor's address (solvers._cached_plan)
        delta, cg_its, _ = cg_solve(desc.with_(form=3, noise=s_ref, obs_w=w), rhs, tol=cg_tol, stop_mode=1,
                                    jacobi=sampling.OBSERVED_JACOBI[0], max_iter=max_iter)
        return delta, cg_its

    with torch.no_grad():
        zero = torch.zeros(desc.n, dtype=torch.float32, device=dev)
        start = None if f0 is None else _lib.f32c(f0.to(dev).reshape(-1))
        f, _, sums, converged, its, history = _newton(name, evaluate, lambda v: _q2(desc, v), solve, zero, start, rtol, max_newton,
                                                      step_tol)
    return f, sums, converged, its, history


# ------------------------------------------------------------------------------------------------ C classes: softmax
MAX_CLASSES = 64


def _block(t, n, C, name):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != n or t.shape[1] != C:
        raise ValueError("%s must be a tensor [%d, %d], got %s" % (name, n, C, tuple(t.shape) if torch.is_tensor(t) else type(t)))
    return _lib.f32c(t)


def _classes(num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= MAX_CLASSES:
        raise ValueError("num_classes must be an int in 2 .. %d, got %r" % (MAX_CLASSES, num_classes))
    return num_classes


def softmax_site(f, qf, labels, observed=None):
    """(pi, rhs, sums) of mgp_softmax_site as fresh tensors: pi = softmax(f) row by row (rows of zeros at unobserved nodes)
    and rhs = onehot(labels) - pi - qf, float32 [n, C]; sums [4] float64 on the device (sum_obs log p, sum f . qf,
    max |rhs|, sum rhs^2).  f [n, C] float32, 2 <= C <= 64; qf [n, C] or None (zeros); labels [n] int32, read at the
    observed nodes; observed [n] bool or None (every node)."""
    if not torch.is_tensor(f) or f.dim() != 2:
        raise ValueError("f must be a tensor [n, C]")
    n, C = f.shape
    _classes(int(C))
    if n < 1:
        raise ValueError("f has no rows")
    if qf is not None:
        qf = _block(qf, n, C, "qf")
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.dim() != 1 or labels.shape[0] != n:
        raise ValueError("labels must be an int32 tensor [%d]" % n)
    if observed is not None and (not torch.is_tensor(observed) or observed.dtype != torch.bool or observed.dim() != 1
                                 or observed.shape[0] != n):
        raise ValueError("observed must be a bool tensor [%d]" % n)
    _lib.require_device(f, qf, labels, observed)
    f, labels = _lib.f32c(f), labels.contiguous()
    observed = None if observed is None else observed.contiguous()
    pi, rhs = torch.empty_like(f), torch.empty_like(f)
    sums = torch.empty(4, dtype=torch.float64, device=f.device)
    wb = lib().mgp_softmax_site_workspace_bytes(n, C)
    work = _lib.workspace(wb, "softmax_site", f.device)
    check(lib().mgp_softmax_site(ptr(f), ptr(qf), ptr(labels), ptr(observed), n, C, ptr(pi), ptr(rhs), ptr(sums), ptr(work),
                                 work.numel(), stream()), "mgp_softmax_site")
    return pi, rhs, sums


def softmax_hessian_add(pi, X, Y):
    """Y += H(pi) X in place, (H X)_i = pi_i o x_i - pi_i (pi_i . x_i): mgp_softmax_hessian_add, the epilogue of a step of
    softmax_cg_solve.  pi, X, Y [n, C] float32 contiguous on the device, X and Y distinct.  Returns Y."""
    if not torch.is_tensor(pi) or pi.dim() != 2:
        raise ValueError("pi must be a tensor [n, C]")
    n, C = pi.shape
    _classes(int(C))
    for name, t in (("pi", pi), ("X", X), ("Y", Y)):
        if not torch.is_tensor(t) or t.shape != pi.shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float32 tensor [%d, %d]" % (name, n, C))
    _lib.require_device(pi, X, Y)
    check(lib().mgp_softmax_hessian_add(ptr(pi), ptr(X), n, C, ptr(Y), stream()), "mgp_softmax_hessian_add")
    return Y


def softmax_noise_factor(pi, eps):
    """R eps with R_i R_i^T = H_i = diag(pi_i) - pi_i pi_i^T (the rows of pi sum to 1 or are 0):
    (R eps)_ic = sqrt(pi_ic) eps_ic - pi_ic sum_k sqrt(pi_ik) eps_ik.  pi, eps [n, C]; the dtype of eps."""
    root = pi.to(eps.dtype).sqrt()
    return root * eps - pi.to(eps.dtype) * (root * eps).sum(-1, keepdim=True)


def _check_cg_args(tol, max_iter, check_every):
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError("max_iter must be a positive int, got %r" % (max_iter,))
    if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
        raise ValueError("check_every must be a positive int, got %r" % (check_every,))
    if not tol >= 0.0:
        raise ValueError("tol must be >= 0, got %r" % (tol,))


def softmax_cg_solve(desc, pi, rhs, tol=1e-3, max_iter=5000, check_every=8):
    """Solve (Q2 (x) I_C + H(pi)) X = rhs as one system of size n C (mgp_softmax_cg): (X [n, C] float32, iterations, relative
    residual of the recurrence).  desc: a form-0 precision descriptor; pi, rhs [n, C].  Where the graph has a locality order
    the solve runs on the relabelled descriptor, rows permuted in and out, as cg_solve does.  Warns when max_iter is reached,
    raises on a non-finite residual."""
    from .solvers import RELABEL_SOLVES
    if int(desc.form) != 0:
        raise NotImplementedError("softmax_cg_solve needs a form-0 precision descriptor")
    if not torch.is_tensor(pi) or pi.dim() != 2 or pi.shape[0] != desc.n:
        raise ValueError("pi must be a tensor [%d, C]" % desc.n)
    n, C = pi.shape
    _classes(int(C))
    pi, rhs = _block(pi, n, C, "pi"), _block(rhs, n, C, "rhs")
    _check_cg_args(tol, max_iter, check_every)
    _lib.require_device(pi, rhs)
    rg = None
    if RELABEL_SOLVES[0]:
        rdesc, rg = desc.relabelled()
        if rdesc is not None:
            desc, pi, rhs = rdesc, rg.permute(pi).contiguous(), rg.permute(rhs).contiguous()
        else:
            rg = None
    op = desc.struct()
    X = torch.empty_like(rhs)
    wb = lib().mgp_softmax_cg_workspace_bytes(ctypes.byref(op), C)
    if wb == 0:
        raise RuntimeError("mgp_softmax_cg_workspace_bytes: unsupported operator / class count %d" % C)
    work = _lib.workspace(wb, "softmax_cg", rhs.device)
    iters, status, resid = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_float(0.0)
    check(lib().mgp_softmax_cg(ctypes.byref(op), ptr(pi), C, ptr(rhs), ptr(X), float(tol), max_iter, check_every,
                               ctypes.byref(iters), ctypes.byref(resid), ctypes.byref(status), ptr(work), work.numel(),
                               stream()), "mgp_softmax_cg")
    if status.value == 2:
        warnings.warn("CG did not converge in %d iterations (residual %.3g)" % (iters.value, resid.value))
    elif status.value == 3:
        raise RuntimeError("NaNs encountered in CG")
    if rg is not None:
        X = rg.unpermute(X)
    return X, int(iters.value), float(resid.value)


MAX_BLOCK_COLUMNS = sampling.CHUNK       # S C <= 256: the operator path's column cap


def _block_width(block, C):
    """`block` of latent_samples / predict_proba / latent_variance: None (one solve per sample) or the samples per solve."""
    if block is None:
        return None
    if isinstance(block, bool) or not isinstance(block, int) or block < 1:
        raise ValueError("block must be None or a positive int, got %r" % (block,))
    if block * C > MAX_BLOCK_COLUMNS:
        raise ValueError("block = %d samples of %d classes are %d columns: the limit is %d" % (block, C, block * C,
                                                                                            MAX_BLOCK_COLUMNS))
    return block


def softmax_cg_solve_block(desc, pi, rhs, tol=1e-3, max_iter=5000, check_every=8):
    """Solve (Q2 (x) I_C + H(pi)) X_s = rhs_s for the S right-hand sides rhs [n, S, C] in one block (mgp_softmax_cg_block):
    (X [n, S, C] float32, iterations per sample, relative residual of each sample's recurrence).  Every sample runs the CG of
    softmax_cg_solve with its own scalars and stops updating when its residual is <= tol; the operator chain runs once per step
    on the S C <= 256 columns.  desc and pi [n, C] as softmax_cg_solve; the solve runs on the relabelled descriptor, rows
    permuted in and out, and from 48 columns on it takes the matrix-core tile SpMM on the chain-relabelled matrix where the
    graph has one, as cg_solve does.  Warns when max_iter is reached, naming the samples above tol; raises on a non-finite
    residual."""
    from .solvers import RELABEL_SOLVES
    if int(desc.form) != 0:
        raise NotImplementedError("softmax_cg_solve_block needs a form-0 precision descriptor")
    if not torch.is_tensor(pi) or pi.dim() != 2 or pi.shape[0] != desc.n:
        raise ValueError("pi must be a tensor [%d, C]" % desc.n)
    n, C = pi.shape
    _classes(int(C))
    if not torch.is_tensor(rhs) or rhs.dim() != 3 or rhs.shape[0] != n or rhs.shape[1] < 1 or rhs.shape[2] != C:
        raise ValueError("rhs must be a tensor [%d, S, %d], got %s" % (n, C, tuple(rhs.shape) if torch.is_tensor(rhs) else type(rhs)))
    S = int(rhs.shape[1])
    if S * C > MAX_BLOCK_COLUMNS:
        raise ValueError("rhs holds S C = %d x %d = %d columns: the limit is %d" % (S, C, S * C, MAX_BLOCK_COLUMNS))
    pi, rhs = _block(pi, n, C, "pi"), _lib.f32c(rhs)
    _check_cg_args(tol, max_iter, check_every)
    _lib.require_device(pi, rhs)
    rg = None
    wide = S * C >= 48               # 48 columns and more: the matrix-core tile SpMM on the chain-relabelled matrix, as CgPlan
    if RELABEL_SOLVES[0]:
        rdesc, rg = desc.relabelled(wide=wide)
        if rdesc is not None:
            desc, pi, rhs = rdesc, rg.permute(pi).contiguous(), rg.permute(rhs.view(n, S * C)).contiguous().view(n, S, C)
        else:
            rg = None
    op = desc.struct(wide=wide)
    X = torch.empty_like(rhs)
    wb = lib().mgp_softmax_cg_block_workspace_bytes(ctypes.byref(op), C, S)
    if wb == 0:
        raise RuntimeError("mgp_softmax_cg_block_workspace_bytes: unsupported operator / %d samples of %d classes" % (S, C))
    work = _lib.workspace(wb, "softmax_cg_block", rhs.device)
    iters, resid, status = (ctypes.c_int32 * S)(), (ctypes.c_float * S)(), ctypes.c_int32(0)
    check(lib().mgp_softmax_cg_block(ctypes.byref(op), ptr(pi), C, S, ptr(rhs), ptr(X), float(tol), max_iter, check_every, iters,
                                     resid, ctypes.byref(status), ptr(work), work.numel(), stream()), "mgp_softmax_cg_block")
    iters, resid = [int(v) for v in iters], [float(v) for v in resid]
    if status.value == 2:
        late = [k for k in range(S) if not resid[k] <= tol]
        warnings.warn("CG did not converge in %d iterations: samples %s of the block are above tol (largest residual %.3g)"
                      % (max(iters), late, max(resid)))
    elif status.value == 3:
        raise RuntimeError("NaNs encountered in CG")
    if rg is not None:
        X = rg.unpermute(X.view(n, S * C)).view(n, S, C)
    return X, iters, resid


def _validate_multiclass(desc, labels, num_classes, observed, f0):
    """The host-side argument checks of laplace_fit_multiclass: (labels [n] int32, observed [n] bool or None), on whatever
    device they came."""
    sampling._check_desc(desc)
    C = _classes(num_classes)
    n = desc.n
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.shape[0] != n or labels.dtype == torch.bool:
        raise ValueError("labels must be a tensor of %d class indices, got %s"
                         % (n, tuple(labels.shape) if torch.is_tensor(labels) else type(labels)))
    if _sites.check_mask(observed, n) is not None:
        observed = observed.to(labels.device)
    seen = labels if observed is None else labels[observed]
    if not bool(((seen >= 0) & (seen < C) & (seen == seen.round() if seen.is_floating_point() else True)).all()):
        raise ValueError("labels at the observed nodes must all be integers in [0, %d)" % C)
    if f0 is not None and (not torch.is_tensor(f0) or f0.dim() != 2 or f0.shape[0] != n or f0.shape[1] != C):
        raise ValueError("f0 must be a tensor [%d, %d] of latent values" % (n, C))
    # the observed entries are in [0, C) by now; the rest is never read but has to survive the cast to int32.  Integer labels
    # are widened first: clamp(-1, .) on a uint8 tensor would wrap the bound to 255 and turn every label into MAX_CLASSES
    if labels.is_floating_point():
        labels = torch.nan_to_num(labels, nan=-1.0, posinf=-1.0, neginf=-1.0).clamp(-1.0, float(MAX_CLASSES))
    else:
        labels = labels.to(torch.int64).clamp(-1, MAX_CLASSES)
    return labels.to(torch.int32), observed


class MulticlassLaplaceFit:
    """The Laplace approximation N(mean, (Q2 (x) I + H)^-1) of the latent posterior of C classes (laplace_fit_multiclass).
    mean [n, C] float32: the mode, rows summing to 0 up to the solver's tolerance; converged, iterations; history: one
    (psi, relative gradient, step, CG iterations) per Newton step; log_likelihood: sum_obs log softmax(mean_i)[t_i];
    pi [n, C] float32: softmax(mean) on the observed rows, 0 elsewhere (the weights of H)."""
    family = "multiclass"

    def __init__(self, desc, labels, observed, mean, pi, converged, iterations, history, log_likelihood):
        self.desc, self.labels, self.observed = desc, labels, observed
        self.mean, self.pi, self.converged, self.iterations = mean, pi, converged, iterations
        self.history, self.log_likelihood = history, log_likelihood

    @property
    def num_classes(self):
        return self.mean.shape[1]

    def map_proba(self):
        """softmax(mean) row by row: the class probabilities at the mode, [n, C] float64 (ignores the latent variance)."""
        return torch.softmax(self.mean.double(), dim=-1)

    def evidence(self, **kw):
        raise NotImplementedError("the evidence of the softmax fit has its own entry point: MulticlassLaplaceFit.laplace_evidence "
                                  "(evidence.softmax_evidence)")

    def laplace_evidence(self, **kw):
        """log Z of this fit and, with operator=, its hyper-parameter gradient: evidence.softmax_evidence(self, **kw)."""
        from .evidence import softmax_evidence
        return softmax_evidence(self, **kw)

    def _delta_blocks(self, S, seed, tol, max_iter, b):
        """The deviations delta_s = A^-1 (z_s + R eps_s) ~ N(0, A^-1) of the samples s = 0 .. S - 1, `b` per solve: (delta
        [n, b, C] float32, the number of live samples in it) per block; the samples beyond S - 1 of the last block are zeros."""
        desc, C = self.desc, self.num_classes
        P = sampling._check_desc(desc)
        _lib.require_device(self.mean, self.pi)
        n, pi = desc.n, self.pi[:, None, :]
        with torch.no_grad():
            for s0 in range(0, S, b):
                # every block has width b, the last one too: sample s then depends on (seed, s, b) alone, not on S
                z = sampling._precision_chunk(desc, P, b * C, seed, s0 * C).view(n, b, C)
                eps = sampling.gmrf_noise(desc.data, b * C, seed, s0 * C, tag=2).view(n, b, C)
                rhs = z + softmax_noise_factor(pi, eps)
                if s0 + b > S:
                    rhs[:, S - s0:] = 0.0
                yield softmax_cg_solve_block(desc, self.pi, rhs, tol=tol, max_iter=max_iter)[0], min(b, S - s0)

    def _samples(self, S, seed, tol, max_iter, block=None):
        """Sample s = 0 .. S - 1 as [n, C] float32: one at a time (block None), or drawn `block` per solve (views into the
        block's [n, block, C] solution, which lives until the next block is drawn)."""
        S, seed = sampling._count(S), sampling._seed(seed)
        desc, C = self.desc, self.num_classes
        b = _block_width(block, C)
        P = sampling._check_desc(desc)
        with torch.no_grad():
            if b is None:
                for s in range(S):
                    z = sampling._precision_chunk(desc, P, C, seed, s * C)
                    eps = sampling.gmrf_noise(desc.data, C, seed, s * C, tag=2)
                    delta = softmax_cg_solve(desc, self.pi, z + softmax_noise_factor(self.pi, eps), tol=tol, max_iter=max_iter)[0]
                    yield self.mean + delta
                return
            for delta, live in self._delta_blocks(S, seed, tol, max_iter, b):
                x = self.mean[:, None, :] + delta
                for k in range(live):
                    yield x[:, k]

    def latent_samples(self, S, seed=None, tol=1e-5, max_iter=5000, block=None):
        """F ~ N(mean, A^-1), A = Q2 (x) I + H: [S, n, C] float32, by perturb-and-MAP on the coupled system:
        delta = A^-1 (z + R eps) with z_c ~ N(0, Q2) independent per class (sampling._precision_chunk) and eps ~ N(0, I)
        (gmrf_noise, tag 2) through softmax_noise_factor.  Sample s takes the noise offsets s C .. s C + C - 1 of both streams:
        it depends on (seed, s) alone.  block None: one softmax_cg_solve per sample, to the relative residual tol.
        block = b (b C <= 256): the samples s0 .. s0 + b - 1 come from one softmax_cg_solve_block on b C columns, every sample to
        the same tol with its own CG scalars; the noise offsets are the same, the SpMM kernel and so the rounding are not:
        sample s then depends on (seed, s, b)."""
        S = sampling._count(S)
        out = torch.empty(S, self.desc.n, self.num_classes, dtype=torch.float32, device=self.mean.device)
        for s, x in enumerate(self._samples(S, seed, tol, max_iter, block)):
            out[s] = x
        return out

    def predict_proba(self, S=64, seed=None, block=None):
        """The mean over S latent samples (latent_samples(S, seed, block=block)) of softmax(F_s) row by row, float64 [n, C]: the
        Monte-Carlo estimate of the class probabilities under the Laplace posterior (rows sum to 1).  The samples are summed as
        they are drawn, in the order s = 0 .. S - 1: O(n C) memory at any S (O(n b C) with block = b)."""
        S, seed = sampling._count(S), sampling._seed(seed)     # (one seed for all samples when it is drawn here)
        acc = torch.zeros(self.desc.n, self.num_classes, dtype=torch.float64, device=self.mean.device)
        for x in self._samples(S, seed, 1e-5, 5000, block):
            acc += torch.softmax(x.double(), dim=-1)
        return acc / S

    def latent_variance(self, S=64, seed=None, block=None):
        """(var, se): the marginal variances diag(A^-1) of the latent posterior as [n, C] and the standard error of the estimate,
        float64 each, from the S samples of latent_samples(S, seed, block=block): delta_s = F_s - mean has mean 0 exactly, so
        var = mean_s delta_s^2 and se = sqrt((mean_s delta_s^4 - var^2) / S).  The plain estimator: its error falls as
        sqrt(2 / S) var; accumulated in float64 as the samples are drawn."""
        S, seed = sampling._count(S), sampling._seed(seed)
        mean = self.mean.double()
        m2, m4 = torch.zeros_like(mean), torch.zeros_like(mean)
        for x in self._samples(S, seed, 1e-5, 5000, block):
            d2 = (x.double() - mean) ** 2
            m2 += d2
            m4 += d2 * d2
        m2, m4 = m2 / S, m4 / S
        return m2, ((m4 - m2 * m2).clamp_min(0.0) / S).sqrt()


def laplace_fit_multiclass(desc, labels, num_classes, observed=None, rtol=1e-5, max_newton=30, cg_tol=1e-3, max_iter=5000,
                           f0=None):
    """The mode of the latent posterior of num_classes (2 .. 64) classes under a softmax likelihood, by Newton's method with
    step halving: MulticlassLaplaceFit.  labels [n]: class indices in [0, num_classes) at the observed nodes (bool [n]; None:
    every node), an integer tensor or a float tensor of whole numbers; the other entries are not read and may be NaN.
    desc: a form-0 precision descriptor as the samplers take; the C latent functions share it as independent priors.
    Stops when max |G - Q2 F| <= rtol times its value at F = 0; every step is one coupled CG solve (softmax_cg_solve) to the
    relative residual cg_tol.  f0 [n, C]: the starting point (default 0)."""
    labels, observed = _validate_multiclass(desc, labels, num_classes, observed, f0)
    _lib.require_device(labels, f0)
    dev = desc.data.graph.device
    n, C = desc.n, num_classes
    labels = labels.to(dev).contiguous()
    obs = None if observed is None else observed.to(dev).contiguous()

    def site(f, qf):
        pi, rhs, sums = softmax_site(f, qf, labels, obs)
        return pi, rhs, sums.tolist()                     # the one host read of an evaluation

    def solve(pi, rhs):
        delta, cg_its, _ = softmax_cg_solve(desc, pi, rhs, tol=cg_tol, max_iter=max_iter)
        return delta, cg_its

    with torch.no_grad():
        zero = torch.zeros(n, C, dtype=torch.float32, device=dev)
        start = None if f0 is None else _lib.f32c(f0.to(dev))
        f, pi, sums, converged, its, history = _newton("laplace_fit_multiclass", site, lambda v: _q2(desc, v), solve, zero,
                                                       start, rtol, max_newton)
    return MulticlassLaplaceFit(desc, labels, obs, f, pi, converged, its, history, sums[0])
