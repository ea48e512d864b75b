"""The Laplace evidence of the node fits and its hyper-parameter gradient (docs/kernels/evidence.md).

With Q the form-0 precision, f the mode of a LaplaceFit / CountLaplaceFit, h = -l''(f) and h' = dh / df (0 off the observed
nodes), A = Q + H, S = diag(sqrt h) and m the observed nodes with h >= H_FLOOR,

    log Z ~= sum_obs l_i(f) - 1/2 f^T Q f - 1/2 logdet B,      B = I + S Q^-1 S,      logdet B = logdet A - logdet Q.

B is the identity off the m nodes and well conditioned where Q is not, so logdet B is Lanczos quadrature on B itself with
Rademacher probes that live on the m nodes (logdet_b, method "slq"), or, for small m, the float64 Cholesky of the m x m block
(method "dense").  A product B V = V + s o Q^-1 (s o V) is one multi-column cg_solve between two mgp_scale_rows launches.

For a kernel hyper-parameter theta with Q' = dQ / d theta (the likelihood's mean, exposure and trials held fixed)

    d log Z / d theta = -1/2 f^T Q' f + 1/2 u^T Q' f + 1/(2 P) sum_p x_p^T Q' y_p
    u = A^-1 (v o h'),  v = diag(A^-1),      X = Q^-1 (s o Z),  Y = A^-1 (s o Z),  Z the probes

every term a bilinear form in Q(theta) between detached vectors: one differentiable operator.matmul of the block [f | Y],
added to the value as sur - sur.detach() the way solvers.inv_quad_logdet does.

The ordered-category fit (ordinal.OrdinalLaplaceFit) has the same evidence with its own site stage (mgp_ordinal_evidence_site: the
node's interval of cutpoints in the place of the observation) and one more set of parameters, the cutpoints b: d log Z / d b_k
is three per-cutpoint sums over the nodes (mgp_ordinal_cut_sums, docs/kernels/ordinal.md) of the same v and u, with no trace
estimate, and enters the value as the surrogate (G . b).  The negative-binomial count fit has one more parameter too, its
dispersion r: d log Z / dr is three sums over the nodes of the same v and u (mgp_nb_dispersion_sums, docs/kernels/counts.md) and
enters the value as (G r).

The C-class softmax fit (classification.MulticlassLaplaceFit) has a Hessian that is not diagonal; its evidence, with the block
factor R in the place of S and a curvature term accumulated from latent samples, is the last part of this module
(softmax_evidence, logdet_b_softmax; mgp_softmax_root_apply and mgp_softmax_curvature).
"""
import math

import numpy as np
import torch

from . import _lib, _sites, families, sampling
from ._lib import check, lib, ptr, stream
from .classification import H_FLOOR

FAMILIES = families.codes("evidence", own=False)           # the families of mgp_laplace_evidence_site
NB_FAMILY = families.with_own("nb")        # the family with an entry point of its own (mgp_nb_evidence_site)
NB = families.TABLE[NB_FAMILY].evidence
ORDINAL_FAMILY = families.with_own("ordinal")   # the ordered-category fit: intervals of cutpoints, not (y, aux) (mgp_ordinal_evidence_site)
DENSE_MAX = 512           # method "auto": the m x m Cholesky up to here
MAX_COLUMNS = sampling.CHUNK


def evidence_site(f, y, aux, observed, variance, mean, family, h_floor=H_FLOOR, dispersion=None):
    """(root_h, corr, sums) of mgp_laplace_evidence_site at the mode f [n] float32: root_h = sqrt(h) and corr = variance h' as
    fresh float32 [n] tensors (0 off the observed nodes with h >= h_floor; corr None when variance is None), sums [4] float64 on
    the device (sum_obs l without the f-independent constant, m = nodes kept, sum corr, max |corr|).  y [n]; aux [n]: the
    log-exposure (family "poisson" and "negative_binomial", the latter with its dispersion, mgp_nb_evidence_site; None: zeros) or
    the trials ("binomial"); family "bernoulli" reads y as labels and takes no aux; observed [n] bool or None (every node); variance [n] (taken as float64) or None; mean: the constant of the linear
    predictor."""
    rec = families._family(family, "evidence")
    r = families.check_dispersion(rec, dispersion)
    if rec.aux == "trials" and aux is None:
        raise ValueError("the binomial family needs the trials in aux")
    if rec.aux is None and aux is not None:
        raise ValueError("the bernoulli family takes no aux")
    site, name, workspace_bytes, code = families.stage(rec, "evidence_site", r)
    f, (y, aux), observed, variance, n, root_h, corr, sums, work = _sites.evidence_args(
        f, (("y", y),), (("aux", aux),), observed, variance, h_floor, workspace_bytes)
    check(site(ptr(f), ptr(y), ptr(aux), ptr(observed), ptr(variance), n, float(mean), code, float(h_floor), ptr(root_h), ptr(corr),
               ptr(sums), ptr(work), work.numel(), stream()), name)
    return root_h, corr, sums


def scale_rows(s, V, X=None, out=None):
    """out = s_i V_ij (X None) or fmaf(s_i, X_ij, V_ij) on float32 blocks [n, P], P <= 256 (mgp_scale_rows).  s [n]; V, X, out
    contiguous float32 [n, P]; out (default: a fresh tensor) may be V or X.  Returns out."""
    if not torch.is_tensor(V) or V.dim() != 2 or V.dtype != torch.float32 or not V.is_contiguous():
        raise ValueError("V must be a contiguous float32 tensor [n, P]")
    n, P = V.shape
    if n < 1 or not 1 <= P <= MAX_COLUMNS:
        raise ValueError("V is [%d, %d]: n >= 1 and 1 <= P <= %d" % (n, P, MAX_COLUMNS))
    if not torch.is_tensor(s) or s.numel() != n:
        raise ValueError("s must be a tensor of %d row factors" % n)
    for name, t in (("X", X), ("out", out)):
        if t is not None and (not torch.is_tensor(t) or t.shape != V.shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 tensor [%d, %d]" % (name, n, P))
    _lib.require_device(s, V, X, out)
    s = _lib.f32c(s.reshape(-1))
    out = torch.empty_like(V) if out is None else out
    check(lib().mgp_scale_rows(ptr(s), ptr(V), ptr(X), n, P, ptr(out), stream()), "mgp_scale_rows")
    return out


class _BOperator:
    """V -> B V = V + s o Q^-1 (s o V): the `matmul` the generic block Lanczos calls.  Counts its solves' CG iterations."""

    def __init__(self, desc, root_h, solve_tol, max_iter):
        self.desc, self.s = desc, root_h
        self.kw = dict(tol=float(solve_tol), stop_mode=1, max_iter=int(max_iter))
        self.shape = (desc.n, desc.n)
        self.solves = self.iterations = 0
        self._rhs = None

    def solve(self, V):
        """Q^-1 V as a fresh float32 tensor"""
        from .solvers import cg_solve
        X, its, _ = cg_solve(self.desc, V, **self.kw)
        self.solves += 1
        self.iterations += int(its)
        return _lib.f32c(X)

    def matmul(self, V):
        # s o V lands in one buffer kept between the steps, the second scaling overwrites the solve's own result: the two
        # launches allocate nothing
        V = _lib.f32c(V)
        if self._rhs is None or self._rhs.shape != V.shape:
            self._rhs = torch.empty_like(V)
        X = self.solve(scale_rows(self.s, V, out=self._rhs))
        if X.data_ptr() == self._rhs.data_ptr():          # (a solve that handed its input back: never the case today)
            X = X.clone()
        return scale_rows(self.s, V, X, out=X)


def effective_probes(root_h, num_probes, seed):
    """[n, num_probes] float32 on root_h's device: +-1 from a seeded CPU generator on the nodes with root_h > 0, exactly 0
    elsewhere (||z||^2 = m)."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    Z = torch.randint(0, 2, (root_h.numel(), int(num_probes)), generator=gen).float() * 2 - 1
    return Z.to(root_h.device) * (root_h.reshape(-1, 1) > 0).float()


def _positive_int(v, name):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError("%s must be a positive int, got %r" % (name, v))
    return v


def _check_logdet_args(desc, root_h, m, num_probes, steps, solve_tol, method, probes):
    sampling._check_desc(desc)
    n = desc.n
    if not torch.is_tensor(root_h) or root_h.numel() != n:
        raise ValueError("root_h must be a tensor of %d values" % n)
    _positive_int(m, "m")
    if m > n:
        raise ValueError("m = %d exceeds the %d nodes" % (m, n))
    _positive_int(num_probes, "num_probes")
    _positive_int(steps, "steps")
    if not float(solve_tol) > 0.0:
        raise ValueError("solve_tol must be positive, got %r" % (solve_tol,))
    if method not in ("auto", "slq", "dense"):
        raise ValueError("method must be 'auto', 'slq' or 'dense', got %r" % (method,))
    if probes is not None and (not torch.is_tensor(probes) or probes.dim() != 2 or probes.shape[0] != n or probes.shape[1] < 2):
        raise ValueError("probes must be a tensor [%d, P] with P >= 2" % n)


def logdet_b(desc, root_h, m, num_probes=16, steps=12, seed=1337, solve_tol=1e-6, method="auto", probes=None, max_iter=5000):
    """(value, se, per_probe) of logdet B, B = I + S Q^-1 S with S = diag(root_h) (0 off the m effective nodes).
    method "slq": value = mean of per_probe, per_probe_p = m e_1^T log(T_p) e_1 from `steps` Lanczos steps on B started at probe p
    (slq._lanczos_block_generic in batches of <= 16 probes; every product one cg_solve on form 0 to the relative residual
    solve_tol between two scale_rows), se = the sample standard deviation of per_probe / sqrt(P).  probes [n, P] (default:
    effective_probes(root_h, num_probes, seed)) must be +-1 on the effective nodes and 0 elsewhere.
    method "dense": exact up to the solves: the m columns Q^-1 (s o e_j) in chunks of <= 256, float64 Cholesky of the m x m B;
    se = 0, per_probe None.  "auto": dense for m <= 512."""
    _check_logdet_args(desc, root_h, m, num_probes, steps, solve_tol, method, probes)
    _lib.require_device(root_h, probes)
    root_h = _lib.f32c(root_h.reshape(-1))
    if method == "auto":
        method = "dense" if m <= DENSE_MAX else "slq"
    op = _BOperator(desc, root_h, solve_tol, max_iter)
    with torch.no_grad():
        if method == "dense":
            eff = torch.nonzero(root_h > 0).reshape(-1)
            if eff.numel() != m:
                raise ValueError("root_h has %d positive entries, m = %d" % (eff.numel(), m))
            s_eff = root_h[eff].double()
            B = torch.empty(m, m, dtype=torch.float64, device=root_h.device)
            for c0 in range(0, m, MAX_COLUMNS):
                cols = eff[c0:c0 + MAX_COLUMNS]
                E = torch.zeros(desc.n, cols.numel(), dtype=torch.float32, device=root_h.device)
                E[cols, torch.arange(cols.numel(), device=root_h.device)] = root_h[cols]
                B[:, c0:c0 + cols.numel()] = s_eff.view(-1, 1) * op.solve(E)[eff].double()
            B = 0.5 * (B + B.t()) + torch.eye(m, dtype=torch.float64, device=root_h.device)
            value = 2.0 * float(torch.linalg.cholesky(B).diagonal().log().sum())
            return value, 0.0, None
        from .slq import _lanczos_block_generic, _quadrature_log_each
        Z = effective_probes(root_h, num_probes, seed) if probes is None else _lib.f32c(probes)
        P = Z.shape[1]
        k = min(int(steps), m)
        per = []
        for c0 in range(0, P, 16):
            a, b = _lanczos_block_generic(op, Z[:, c0:c0 + 16].contiguous(), k)
            per.append(_quadrature_log_each(a, b))
        per = m * np.concatenate(per)
    value = float(per.mean())
    se = float(per.std(ddof=1) / math.sqrt(P)) if P > 1 else float("nan")
    return value, se, per


class LaplaceEvidence:
    """The Laplace evidence of a node fit (laplace_evidence).  value: log Z as a float64 torch scalar on the device, carrying the
    gradient surrogate when it was asked for; se: its standard error (logdet_se / 2); log_likelihood: sum_obs log p(y_i | f_i)
    with the constants; quad: f^T Q f / 2; logdet: logdet B with logdet_se; method: "slq" or "dense"; m: the effective observed
    nodes; per_probe: the probes' estimates of logdet B (slq); solves: None, or with the gradient the dict of what it was made
    of (Z, root_h, corr, w, s_ref, Y float32; u, X float64; with the cutpoints' gradient alone: root_h, corr, w, s_ref, u);
    site_sums: the four sums of mgp_laplace_evidence_site (sum_obs l without the families' constants, m, sum corr, max |corr|);
    cutpoint_grad: None, or for an ordinal fit asked for the cutpoints' gradient the three rows [3, K - 1] float64 of
    mgp_ordinal_cut_sums on the device, whose column sum is d log Z / d b; dispersion_grad: None, or for a negative-binomial fit
    asked for the dispersion's gradient the three rows [3] float64 of mgp_nb_dispersion_sums on the device, whose sum is
    d log Z / dr."""

    def __init__(self, value, se, log_likelihood, quad, logdet, logdet_se, method, m, per_probe, solves, dispersion_grad=None,
                 site_sums=None, cutpoint_grad=None):
        self.dispersion_grad = dispersion_grad
        self.value, self.se, self.log_likelihood, self.quad = value, se, log_likelihood, quad
        self.logdet, self.logdet_se, self.method, self.m = logdet, logdet_se, method, m
        self.per_probe, self.solves, self.site_sums, self.cutpoint_grad = per_probe, solves, site_sums, cutpoint_grad

    def __repr__(self):
        return "LaplaceEvidence(value=%.6f, se=%.3g, method=%r, m=%d)" % (float(self.value), self.se, self.method, self.m)


def _site_of(fit):
    """(family, mean, aux, s_ref, dispersion) of a binary, a count or an ordinal fit: what the site kernels of its family read
    beside the observations (a fit without a mean, an aux or a dispersion carries 0 and None, classification.LaplaceFit)."""
    return fit.family, fit.prior_mean, fit._aux, fit.s_ref, fit.dispersion


REFINE_ROUNDS = 4         # refinement rounds of the float64 solves of the gradient (they stop at a true residual of 2 tol)


def _solve64(desc, B, kw):
    """A^-1 B as the float64 solution a refined plan accumulates (CgPlan.solution64_view), [n, C] with C <= 256, in the caller's
    order; its true residual on the float64 matrix is <= 2 tol where the plan reports convergence."""
    import warnings
    from .solvers import _cached_plan
    B = _lib.f32c(B)
    plan = _cached_plan(desc, B.shape[1], kw)
    plan.solve(B, copy=False)
    if plan.status == 3:
        raise RuntimeError("NaNs encountered in CG")
    if plan.status == 2:
        warnings.warn("CG did not converge in %d iterations (residuals up to %.3g)" % (plan.iters, max(plan.resid)))
    return plan.solution64_view().clone()


def _check_cutpoints(fit, family, cutpoints):
    """True when the cutpoints' gradient is asked for: cutpoints a float64 [K - 1] tensor that requires grad and rounds to the
    fit's own cutpoints in float32."""
    if cutpoints is None:
        return False
    if families.TABLE[family].extra != "cutpoints":
        raise ValueError("cutpoints belong to an ordinal fit, this is a %s fit" % family)
    K = fit.num_categories
    if not torch.is_tensor(cutpoints) or cutpoints.dtype != torch.float64 or cutpoints.shape != (K - 1,):
        raise ValueError("cutpoints must be a float64 tensor of %d values" % (K - 1))
    if not torch.equal(cutpoints.detach().float().double().cpu(), fit.cutpoints.cpu()):
        raise ValueError("cutpoints are not the fit's: rounded to float32 they must equal fit.cutpoints")
    return bool(cutpoints.requires_grad)


def _check_dispersion(fit, family, dispersion):
    """True when the dispersion's gradient is asked for: dispersion a 0-dim float64 tensor that requires grad and equals the
    fit's own."""
    if dispersion is None:
        return False
    if families.TABLE[family].extra != "dispersion":
        raise ValueError("dispersion belongs to a negative_binomial fit, this is a %s fit" % family)
    if not torch.is_tensor(dispersion) or dispersion.dtype != torch.float64 or dispersion.dim() != 0:
        raise ValueError("dispersion must be a 0-dim float64 tensor")
    if float(dispersion.detach()) != fit.dispersion:
        raise ValueError("dispersion is not the fit's: %r against fit.dispersion = %r" % (float(dispersion.detach()), fit.dispersion))
    return bool(dispersion.requires_grad)


def laplace_evidence(fit, operator=None, variance=None, var_samples=64, num_probes=16, steps=12, seed=1337, solve_tol=1e-6,
                     method="auto", probes=None, max_iter=5000, dispersion=None, cutpoints=None):
    """log Z of a LaplaceFit, a CountLaplaceFit or an OrdinalLaplaceFit: a LaplaceEvidence.
    logdet B by logdet_b(num_probes, steps, seed, solve_tol,
    method, probes).  operator: the model's precision(noise=False), the operator fit.desc describes; when one of its
    _hyper_tensors() requires grad, value carries d log Z / d theta of the module docstring: corr = variance h' from variance
    [n] (default fit.latent_variance(var_samples)[0]), X by one form-0 solve and Y, u by form-3 solves with the fit's s_ref and
    weights, all refined to solve_tol on the true residual (X and u kept as the float64 solutions, _solve64), the probes those
    of logdet B (drawn from num_probes and seed also when method is "dense").
    cutpoints (ordinal fits only): a float64 tensor [K - 1] whose float32 rounding is fit.cutpoints, for example the output of an
    ordinal.CutpointParameter; when it requires grad, value carries d log Z / d b as the surrogate (G . cutpoints) with G the
    column sum of mgp_ordinal_cut_sums (LaplaceEvidence.cutpoint_grad holds the three rows): it needs the variance and the u solve
    of the hyper-parameter gradient, and neither probes nor X and Y.
    dispersion (negative-binomial fits only): a 0-dim float64 tensor equal to fit.dispersion, for example the output of a
    counts.DispersionParameter; when it requires grad, value carries d log Z / dr as the surrogate (G dispersion) with G the sum
    of mgp_nb_dispersion_sums (LaplaceEvidence.dispersion_grad holds the three rows), from the same variance and u solve."""
    from .autograd import needs_grad
    from .solvers import cg_solve
    if not hasattr(fit, "_pseudo") or fit.mean.dim() != 1:
        raise NotImplementedError("laplace_evidence takes a binary, a count or an ordinal fit")
    desc = fit.desc
    family, mean, aux, s_ref, r_nb = _site_of(fit)
    grad = operator is not None and needs_grad(*getattr(operator, "_hyper_tensors", lambda: [])())
    cut_grad = _check_cutpoints(fit, family, cutpoints)
    disp_grad = _check_dispersion(fit, family, dispersion)
    with torch.no_grad():
        f = fit.mean
        if (grad or cut_grad or disp_grad) and variance is None:
            variance = fit.latent_variance(var_samples)[0]
        if families.TABLE[family].aux == "interval":      # the node's interval of cutpoints in the place of (y, aux)
            from .ordinal import ordinal_cut_sums, ordinal_evidence_site
            root_h, corr, sums = ordinal_evidence_site(f, fit._lo, fit._hi, fit.observed, variance if grad or cut_grad else None)
        else:
            root_h, corr, sums = evidence_site(f, fit.y, aux, fit.observed, variance if grad or disp_grad else None, mean, family,
                                              dispersion=r_nb)
        sums = sums.tolist()                              # the one host read of the site stage
        m = int(sums[1])
        if m < 1:
            raise RuntimeError("no observed node has a curvature above %g: the latent values have run away" % H_FLOOR)
        quad = 0.5 * float(torch.dot(f.double(), desc.apply_f64(f.double())))
        if method == "auto":
            method = "dense" if m <= DENSE_MAX else "slq"
        Z = None
        if method == "slq" or grad:
            Z = effective_probes(root_h, num_probes, seed) if probes is None else _lib.f32c(probes)
        logdet, logdet_se, per = logdet_b(desc, root_h, m, num_probes, steps, seed, solve_tol, method, Z if method == "slq" else None,
                                          max_iter)
    ll = float(fit.log_likelihood)
    value = torch.tensor(ll - quad - 0.5 * logdet, dtype=torch.float64, device=f.device)
    solves = G = Gr = None
    if grad or cut_grad or disp_grad:
        with torch.no_grad():
            # X and u only weight the operator's output, so they enter the bilinear forms as the float64 solutions the refined
            # solves accumulate: a float32 X cannot hold a true residual of 2 solve_tol on Q itself (its rounding alone leaves
            # 2.4e-6 on the 1546-node dumbbell, cond Q = 1e3; the unrefined factorised solve of the Lanczos products 4.8e-6).
            # Y goes through the float32 operator chain and stays float32 (refined as sampling.posterior_variance solves form 3).
            kw = dict(tol=float(solve_tol), stop_mode=1, max_iter=int(max_iter))
            w = fit._weights()                            # obs_w of the fit's own form-3 system, from its site kernel
            d3 = desc.with_(form=3, noise=s_ref, obs_w=w)
            kw3 = dict(kw, jacobi=sampling.OBSERVED_JACOBI[0])
            if grad:
                SZ = scale_rows(root_h, Z)
                X = _solve64(desc, SZ, dict(kw, refine=REFINE_ROUNDS))
                Y = cg_solve(d3, SZ * s_ref, **dict(kw3, refine=1))[0]
            # u = A^-1 (v o h') serves every gradient: one solve
            u = _solve64(d3, (corr * s_ref).view(-1, 1), dict(kw3, refine=REFINE_ROUNDS)).view(-1)
            solves = dict(root_h=root_h, corr=corr, w=w, s_ref=s_ref, u=u)
            if cut_grad:
                G = ordinal_cut_sums(f, fit._lo, fit._hi, fit.y, fit.observed, variance, u, fit.num_categories)
            if disp_grad:
                from .counts import nb_dispersion_sums
                Gr = nb_dispersion_sums(f, fit.y, aux, fit.observed, variance, u, mean, r_nb)
            if grad:
                P = Z.shape[1]
                V = torch.cat([f.view(-1, 1), Y], 1).contiguous()
                W = torch.cat([0.5 * (u - f.double()).view(-1, 1), X * (0.5 / P)], 1)
                solves = dict(Z=Z, root_h=root_h, corr=corr, w=w, s_ref=s_ref, u=u, X=X, Y=Y)
    if grad:
        sur = (W * operator.matmul(V).double()).sum()
        value = value + (sur - sur.detach())
    if cut_grad:
        sur = (G.sum(0).to(cutpoints.device) * cutpoints).sum()
        value = value + (sur - sur.detach()).to(value.device)
    if disp_grad:
        sur = Gr.sum().to(dispersion.device) * dispersion
        value = value + (sur - sur.detach()).to(value.device)
    return LaplaceEvidence(value, 0.5 * logdet_se, ll, quad, logdet, logdet_se, method, m, per, solves, dispersion_grad=Gr,
                           site_sums=sums, cutpoint_grad=G)


# ------------------------------------------------------------------------------------------------ the softmax family
# (docs/kernels/evidence.md, "The softmax family").  The C-class fit's Hessian H_i = diag(pi_i) - pi_i pi_i^T is not diagonal, so
# S = diag(sqrt h) gives way to the block-diagonal R with R_i = diag(s_i)(I - s_i s_i^T), s_i = sqrt(pi_i), R_i R_i^T = H_i:
#
#     log Z ~= sum_obs log pi_{i, t_i} - 1/2 sum_c F_c^T Q F_c - 1/2 logdet B,      B = I + R^T (Q^-1 (x) I_C) R
#
# and logdet B = logdet A - C logdet Q with A = Q (x) I_C + H.  B is symmetric positive definite, the identity off the m observed
# rows, and has one exact unit eigenvalue per observed row (along s_i).  A Lanczos vector is a whole [n, C] block; b of them lie
# as [n, C, b], sample fastest: at once an [n, C b] right-hand-side block of cg_solve and an [n C, b] block of the generic block
# Lanczos.  The gradient is that of the module docstring with v o h' replaced by g_ic = tr(V_i dH_i / df_ic), V_i the C x C
# diagonal block of A^-1, which mgp_softmax_curvature accumulates from latent deviations.
MULTICLASS_FAMILY = families.with_own("softmax")
DENSE_MAX_ENTRIES = 4096  # method "auto": the m C x m C Cholesky up to here (128 MiB of float64)
LAYOUTS = ("cs", "sc")    # [n, C, S] (a block of Lanczos vectors) and [n, S, C] (the coupled block solver's)


def _pi_block(pi):
    from .classification import MAX_CLASSES
    if not torch.is_tensor(pi) or pi.dim() != 2 or pi.dtype != torch.float32 or not pi.is_contiguous():
        raise ValueError("pi must be a contiguous float32 tensor [n, C]")
    n, C = pi.shape
    if n < 1 or not 2 <= C <= MAX_CLASSES:
        raise ValueError("pi is [%d, %d]: n >= 1 and 2 <= C <= %d" % (n, C, MAX_CLASSES))
    return int(n), int(C)


def softmax_root_apply(pi, V, X=None, transpose=False, out=None, layout="cs"):
    """R V (transpose False) or V + R^T X (transpose True; V None: R^T X) for the factor R of the softmax Hessian,
    R_i = diag(s_i)(I - s_i s_i^T) with s_i = sqrt(pi_i) (mgp_softmax_root_apply): (R v)_c = s_c v_c - pi_c sum_k s_k v_k and
    (R^T x)_c = s_c (x_c - sum_k pi_k x_k).  pi [n, C] contiguous float32; V, X, out contiguous float32 blocks of S vectors,
    [n, C, S] (layout "cs") or [n, S, C] ("sc"), C S <= 256; out (default: a fresh tensor) may be V or X.  Returns out."""
    n, C = _pi_block(pi)
    if layout not in LAYOUTS:
        raise ValueError("layout must be 'cs' ([n, C, S]) or 'sc' ([n, S, C]), got %r" % (layout,))
    lead = X if transpose else V
    if transpose and X is None:
        raise ValueError("the transposed product needs X")
    if not transpose and X is not None:
        raise ValueError("the forward product R V takes no X")
    if not torch.is_tensor(lead) or lead.dim() != 3 or lead.shape[0] != n or lead.shape[1 if layout == "cs" else 2] != C:
        raise ValueError("%s must be a tensor %s" % ("X" if transpose else "V", "[%d, %d, S]" % (n, C) if layout == "cs"
                                                     else "[%d, S, %d]" % (n, C)))
    S = int(lead.shape[2 if layout == "cs" else 1])
    if S < 1 or C * S > MAX_COLUMNS:
        raise ValueError("%d vectors of %d classes are %d columns: 1 .. %d" % (S, C, C * S, MAX_COLUMNS))
    for name, t in (("V", V), ("X", X), ("out", out)):
        if t is not None and (not torch.is_tensor(t) or t.shape != lead.shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 tensor %s" % (name, list(lead.shape)))
    _lib.require_device(pi, V, X, out)
    out = torch.empty_like(lead) if out is None else out
    cs, ss = (S, 1) if layout == "cs" else (1, C)
    check(lib().mgp_softmax_root_apply(ptr(pi), ptr(V), ptr(X), n, C, S, cs, ss, 1 if transpose else 0, ptr(out), stream()),
          "mgp_softmax_root_apply")
    return out


def softmax_curvature(pi, delta, acc=None, acc2=None):
    """acc += sum_s g_s and acc2 += sum_s g_s^2 over the S deviations delta [n, S, C] float32 of one block, g_s = pi_c (d_c^2 -
    sum_a pi_a d_a^2) with d = delta_s - (pi . delta_s) (mgp_softmax_curvature): (acc, acc2), float64 [n, C] each (default: fresh
    zeros).  pi [n, C] contiguous float32, C S <= 256.  Rows of zeros in pi are not written."""
    n, C = _pi_block(pi)
    if not torch.is_tensor(delta) or delta.dim() != 3 or delta.shape[0] != n or delta.shape[2] != C or delta.dtype != torch.float32 \
            or not delta.is_contiguous():
        raise ValueError("delta must be a contiguous float32 tensor [%d, S, %d]" % (n, C))
    S = int(delta.shape[1])
    if S < 1 or C * S > MAX_COLUMNS:
        raise ValueError("%d samples of %d classes are %d columns: 1 .. %d" % (S, C, C * S, MAX_COLUMNS))
    if (acc is None) != (acc2 is None):
        raise ValueError("acc and acc2 come together")
    for name, t in (("acc", acc), ("acc2", acc2)):
        if t is not None and (not torch.is_tensor(t) or t.shape != pi.shape or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous float64 tensor [%d, %d]" % (name, n, C))
    if acc is not None and acc.data_ptr() == acc2.data_ptr():
        raise ValueError("acc and acc2 must be distinct")
    _lib.require_device(pi, delta, acc, acc2)
    if acc is None:
        acc, acc2 = (torch.zeros(n, C, dtype=torch.float64, device=pi.device) for _ in range(2))
    check(lib().mgp_softmax_curvature(ptr(pi), ptr(delta), n, C, S, ptr(acc), ptr(acc2), stream()), "mgp_softmax_curvature")
    return acc, acc2


class _SoftmaxBOperator:
    """V -> B V = V + R^T (Q^-1 (x) I_C) (R V) on [n C, b] blocks, b vectors of [n, C] laid out [n, C, b]: the `matmul` the
    generic block Lanczos calls.  One cg_solve on the C b columns between two mgp_softmax_root_apply launches.  Counts its
    solves' CG iterations."""

    def __init__(self, desc, pi, solve_tol, max_iter):
        self.desc, self.pi = desc, pi
        self.n, self.C = int(pi.shape[0]), int(pi.shape[1])
        self.kw = dict(tol=float(solve_tol), stop_mode=1, max_iter=int(max_iter))
        self.shape = (self.n * self.C, self.n * self.C)
        self.solves = self.iterations = 0
        self._rhs = None

    solve = _BOperator.solve

    def matmul(self, V):
        V = _lib.f32c(V)
        if V.dim() != 2 or V.shape[0] != self.n * self.C or self.C * V.shape[1] > MAX_COLUMNS:
            raise ValueError("V must be [%d, b] with %d b <= %d" % (self.n * self.C, self.C, MAX_COLUMNS))
        b = V.shape[1]
        V3 = V.view(self.n, self.C, b)
        if self._rhs is None or self._rhs.shape != V3.shape:
            self._rhs = torch.empty_like(V3)
        X = self.solve(softmax_root_apply(self.pi, V3, out=self._rhs).view(self.n, self.C * b))
        if X.data_ptr() == self._rhs.data_ptr():
            X = X.clone()
        X3 = X.view(self.n, self.C, b)
        return softmax_root_apply(self.pi, V3, X3, transpose=True, out=X3).view(self.n * self.C, b)


def softmax_probes(observed, C, num_probes, seed):
    """[n, C, num_probes] float32 on observed's device: +-1 from a seeded CPU generator on the m C (observed row, class) entries,
    exactly 0 elsewhere (||z||^2 = m C)."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    Z = torch.randint(0, 2, (observed.numel(), int(C), int(num_probes)), generator=gen).float() * 2 - 1
    return Z.to(observed.device) * observed.reshape(-1, 1, 1).float()


def _check_softmax_logdet_args(desc, pi, observed, num_probes, steps, solve_tol, method, probes):
    sampling._check_desc(desc)
    n, C = _pi_block(pi)
    if n != desc.n:
        raise ValueError("pi has %d rows, the graph %d nodes" % (n, desc.n))
    if observed is not None and (not torch.is_tensor(observed) or observed.dtype != torch.bool or observed.dim() != 1
                                 or observed.shape[0] != n):
        raise ValueError("observed must be a bool tensor [%d]" % n)
    _positive_int(num_probes, "num_probes")
    _positive_int(steps, "steps")
    if not float(solve_tol) > 0.0:
        raise ValueError("solve_tol must be positive, got %r" % (solve_tol,))
    if method not in ("auto", "slq", "dense"):
        raise ValueError("method must be 'auto', 'slq' or 'dense', got %r" % (method,))
    if probes is not None and (not torch.is_tensor(probes) or probes.dim() != 3 or probes.shape[0] != n or probes.shape[1] != C
                               or probes.shape[2] < 2):
        raise ValueError("probes must be a tensor [%d, %d, P] with P >= 2" % (n, C))
    return n, C


def _softmax_method(method, m, C):
    if method != "auto":
        return method
    return "dense" if m <= DENSE_MAX and m * C <= DENSE_MAX_ENTRIES else "slq"


def logdet_b_softmax(desc, pi, observed, num_probes=16, steps=12, seed=1337, solve_tol=1e-6, method="auto", probes=None,
                     max_iter=5000):
    """(value, se, per_probe) of logdet B, B = I + R^T (Q^-1 (x) I_C) R with R the factor of the softmax Hessian at pi [n, C]
    (softmax on the observed rows, 0 elsewhere; observed [n] bool or None: every node; m = the observed rows).
    method "slq": value = mean of per_probe, per_probe_p = m C e_1^T log(T_p) e_1 from `steps` Lanczos steps on B started at probe
    p (slq._lanczos_block_generic on [n C, b] blocks, b = min(16, 256 // C) probes at a time; every product one cg_solve on form 0
    with C b columns to the relative residual solve_tol between two softmax_root_apply), se = the sample standard deviation of
    per_probe / sqrt(P).  probes [n, C, P] (default: softmax_probes(observed, C, num_probes, seed)) must be +-1 on the observed
    rows and 0 elsewhere.
    method "dense": exact up to the solves: the m columns Q^-1 e_i at the observed nodes in chunks of <= 256, then
    B_(i,a),(j,b) = delta + (Q^-1)_ij (R_i^T R_j)_ab in float64 and its Cholesky factor; se = 0, per_probe None.  "auto": dense
    for m <= 512 and m C <= 4096."""
    n, C = _check_softmax_logdet_args(desc, pi, observed, num_probes, steps, solve_tol, method, probes)
    _lib.require_device(pi, observed, probes)
    dev = pi.device
    observed = torch.ones(n, dtype=torch.bool, device=dev) if observed is None else observed.to(dev)
    rows = torch.nonzero(observed).reshape(-1)
    m = int(rows.numel())
    if m < 1:
        raise ValueError("observed selects no node")
    method = _softmax_method(method, m, C)
    op = _SoftmaxBOperator(desc, pi, solve_tol, max_iter)
    with torch.no_grad():
        if method == "dense":
            K = torch.empty(m, m, dtype=torch.float64, device=dev)
            for c0 in range(0, m, MAX_COLUMNS):
                cols = rows[c0:c0 + MAX_COLUMNS]
                E = torch.zeros(n, cols.numel(), dtype=torch.float32, device=dev)
                E[cols, torch.arange(cols.numel(), device=dev)] = 1.0
                K[:, c0:c0 + cols.numel()] = op.solve(E)[rows].double()
            K = 0.5 * (K + K.t())
            p = pi[rows].double()
            s = p.sqrt()
            R = torch.diag_embed(s) - p.unsqueeze(2) * s.unsqueeze(1)                       # R_i [c, a] = s_c delta_ca - pi_c s_a
            B = torch.einsum("ica,jcb->iajb", R, R) * K.view(m, 1, m, 1)
            B = B.reshape(m * C, m * C)
            B = 0.5 * (B + B.t()) + torch.eye(m * C, dtype=torch.float64, device=dev)
            return 2.0 * float(torch.linalg.cholesky(B).diagonal().log().sum()), 0.0, None
        from .slq import _lanczos_block_generic, _quadrature_log_each
        Z = softmax_probes(observed, C, num_probes, seed) if probes is None else _lib.f32c(probes)
        P = Z.shape[2]
        k = min(int(steps), m * C)
        b = min(16, MAX_COLUMNS // C)
        per = []
        for c0 in range(0, P, b):
            al, be = _lanczos_block_generic(op, Z[:, :, c0:c0 + b].contiguous().view(n * C, -1), k)
            per.append(_quadrature_log_each(al, be))
        per = m * C * np.concatenate(per)
    value = float(per.mean())
    se = float(per.std(ddof=1) / math.sqrt(P)) if P > 1 else float("nan")
    return value, se, per


def _softmax_apply64(desc, pi64, X):
    """A X in float64 for X [n, S, C]: the float64 operator chain on the S C columns plus H(pi) X in torch."""
    n, S, C = X.shape
    QX = torch.cat([desc.apply_f64(X.reshape(n, S * C)[:, c0:c0 + MAX_COLUMNS]) for c0 in range(0, S * C, MAX_COLUMNS)], 1)
    p = pi64.unsqueeze(1)
    return QX.view(n, S, C) + p * X - p * (p * X).sum(-1, keepdim=True)


def _softmax_solve64(desc, pi, rhs, tol, max_iter):
    """A^-1 rhs for rhs [n, S, C] float64 as the float64 sum of softmax_cg_solve_block solutions: the first solve, then up to
    REFINE_ROUNDS corrections on the float64 true residual, each scaled to unit size per sample, until every sample's true
    relative residual is <= 2 tol (a warning where one is not).  Returns X float64 [n, S, C]."""
    import warnings
    from .classification import softmax_cg_solve_block
    n, S, C = rhs.shape
    b = max(1, MAX_COLUMNS // C)
    pi64 = pi.double()
    out, worst = torch.empty_like(rhs), 0.0
    for s0 in range(0, S, b):
        B = rhs[:, s0:s0 + b].contiguous()
        norm_b = B.pow(2).sum((0, 2)).sqrt()
        X, r = torch.zeros_like(B), B
        for _ in range(REFINE_ROUNDS + 1):
            size = r.abs().amax((0, 2)).clamp_min(1e-300).view(1, -1, 1)
            X += softmax_cg_solve_block(desc, pi, (r / size).float(), tol=float(tol), max_iter=int(max_iter))[0].double() * size
            r = B - _softmax_apply64(desc, pi64, X)
            rel = r.pow(2).sum((0, 2)).sqrt() / norm_b.clamp_min(1e-300)
            if bool((rel <= 2.0 * tol).all()):
                break
        out[:, s0:s0 + b] = X
        worst = max(worst, float(rel.max()))
    if worst > 2.0 * tol:
        warnings.warn("coupled softmax solve: true residual %.3g above 2 x the tolerance %.3g after %d corrections"
                      % (worst, tol, REFINE_ROUNDS))
    return out


def softmax_sampled_curvature(fit, var_samples=64, seed=None, block=None, tol=1e-5, max_iter=5000):
    """(g, se) float64 [n, C]: g_ic = tr(V_i dH_i / df_ic) of a MulticlassLaplaceFit as the mean over var_samples latent deviations
    of the blocks MulticlassLaplaceFit._delta_blocks draws (`block` per solve; default min(16, 256 // C)), accumulated by
    softmax_curvature in O(n C) memory, and the standard error of that mean."""
    from .classification import _block_width
    S, seed = sampling._count(var_samples), sampling._seed(seed)
    C = fit.num_classes
    b = _block_width(block, C) or min(16, MAX_COLUMNS // C)
    acc = acc2 = None
    for delta, _ in fit._delta_blocks(S, seed, tol, max_iter, b):       # (the dead samples of the last block are 0: g_s = 0)
        acc, acc2 = softmax_curvature(fit.pi, delta, acc, acc2)
    g = acc / S
    se = ((acc2 / S - g * g).clamp_min(0.0) / max(S - 1, 1)).sqrt()
    return g, se


def softmax_evidence(fit, operator=None, curvature=None, var_samples=64, block=None, num_probes=16, steps=12, seed=1337,
                     solve_tol=1e-6, method="auto", probes=None, max_iter=5000):
    """log Z of a classification.MulticlassLaplaceFit: a LaplaceEvidence with m = the observed rows, log_likelihood the fit's,
    quad = 1/2 sum_c F_c^T Q F_c from the float64 operator chain and logdet B by logdet_b_softmax(num_probes, steps, seed,
    solve_tol, method, probes).  operator: the model's precision(noise=False), the operator fit.desc describes; when one of its
    _hyper_tensors() requires grad, value carries

        d log Z / d theta = -1/2 sum_c F_c^T Q' F_c + 1/2 sum_c u_c^T Q' F_c + 1/(2 P) sum_p sum_c x_pc^T Q' y_pc
        u = A^-1 g,      X = (Q^-1 (x) I) R Z,      Y = A^-1 R Z,      Z the probes [n, C, P] of logdet B

    as one differentiable operator.matmul of [F | Y] (C (1 + P) columns in chunks of <= 256) weighted in float64.  g [n, C] is
    `curvature` (float64, for example the dense one) or softmax_sampled_curvature(fit, var_samples, seed, block).  X is the
    refined float64 form-0 solve (_solve64), u and Y the float64 sums of _softmax_solve64, all to a true residual of 2 solve_tol;
    Y enters the operator rounded to float32.  solves: None, or dict(Z, u, X, Y, g, g_se) with X, Y [n, C, P]."""
    from .autograd import needs_grad
    if getattr(fit, "family", None) != MULTICLASS_FAMILY:
        raise NotImplementedError("softmax_evidence takes a MulticlassLaplaceFit")
    desc, F, pi = fit.desc, fit.mean, _lib.f32c(fit.pi)
    n, C = _pi_block(pi)
    if curvature is not None and (not torch.is_tensor(curvature) or curvature.shape != pi.shape):
        raise ValueError("curvature must be a tensor [%d, %d]" % (n, C))
    _check_softmax_logdet_args(desc, pi, fit.observed, num_probes, steps, solve_tol, method, probes)
    grad = operator is not None and needs_grad(*getattr(operator, "_hyper_tensors", lambda: [])())
    dev = F.device
    with torch.no_grad():
        observed = torch.ones(n, dtype=torch.bool, device=dev) if fit.observed is None else fit.observed
        m = int(observed.sum())
        F64 = F.double()
        quad = 0.5 * float((F64 * desc.apply_f64(F64)).sum())
        method = _softmax_method(method, m, C)
        Z = None
        if method == "slq" or grad:
            Z = softmax_probes(observed, C, num_probes, seed) if probes is None else _lib.f32c(probes)
        logdet, logdet_se, per = logdet_b_softmax(desc, pi, observed, num_probes, steps, seed, solve_tol, method,
                                                  Z if method == "slq" else None, max_iter)
    ll = float(fit.log_likelihood)
    value = torch.tensor(ll - quad - 0.5 * logdet, dtype=torch.float64, device=dev)
    solves = None
    if grad:
        with torch.no_grad():
            if curvature is None:
                g, g_se = softmax_sampled_curvature(fit, var_samples, seed, block)
            else:
                g, g_se = curvature.to(dev).double(), None
            P = Z.shape[2]
            kw = dict(tol=float(solve_tol), stop_mode=1, max_iter=int(max_iter), refine=REFINE_ROUNDS)
            RZ = torch.cat([softmax_root_apply(pi, Z[:, :, p0:p0 + MAX_COLUMNS // C].contiguous())
                            for p0 in range(0, P, MAX_COLUMNS // C)], 2)                     # [n, C, P]
            flat = RZ.view(n, C * P)
            X = torch.cat([_solve64(desc, flat[:, c0:c0 + MAX_COLUMNS].contiguous(), kw) for c0 in range(0, C * P, MAX_COLUMNS)],
                          1).view(n, C, P)
            both = _softmax_solve64(desc, pi, torch.cat([g.view(n, 1, C), RZ.permute(0, 2, 1).double()], 1), solve_tol, max_iter)
            u, Y = both[:, 0].contiguous(), both[:, 1:].permute(0, 2, 1).contiguous()      # [n, C] and [n, C, P]
            V = torch.cat([F, Y.float().view(n, C * P)], 1).contiguous()
            W = torch.cat([0.5 * (u - F64), X.view(n, C * P) * (0.5 / P)], 1)
            solves = dict(Z=Z, u=u, X=X, Y=Y, g=g, g_se=g_se)
        sur = sum((W[:, c0:c0 + MAX_COLUMNS] * operator.matmul(V[:, c0:c0 + MAX_COLUMNS].contiguous()).double()).sum()
                  for c0 in range(0, V.shape[1], MAX_COLUMNS))
        value = value + (sur - sur.detach())
    return LaplaceEvidence(value, 0.5 * logdet_se, ll, quad, logdet, logdet_se, method, m, per, solves)
