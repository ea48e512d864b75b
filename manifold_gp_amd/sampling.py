"""Exact samples of the Matern graph GP in precision form (docs/kernels/sampling.md).

With A = tau I + L_sym (tau = 2 nu / kappa^2) the precision of a form-0 descriptor is Q2 = scale P A^nu P, P = I
(symmetric normalisation) or D^1/2 (random walk: pre = post = sqrt(D)).  A has the sparse factor
G = [sqrt(tau) I | E] (A = G G^T, one entry of E per edge and endpoint), so with w node noise and g = G w_full:

    z ~ N(0, Q2)                   odd nu: sqrt(scale) P A^((nu-1)/2) g        even nu: sqrt(scale) P A^(nu/2) w
    f ~ N(0, Q2^-1)                odd nu: scale^-1/2 P^-1 A^-((nu+1)/2) g    even nu: scale^-1/2 P^-1 A^-(nu/2) w
    f | y, noise s (perturb-and-MAP):  x = (I + s Q2)^-1 (y + s z + sqrt(s) w2)   [+ sqrt(s) w3 with noisy=True]

Observed subsets / per-node noise (observed=, noise [n]): W = diag(w), w_i = s_ref / sigma_i^2 on observed nodes and 0
elsewhere, s_ref = min over observed sigma_i^2.  Posterior precision Q2 + W / s_ref, system A3 = W + s_ref Q2 (operator form 3):

    mean  x = A3^-1 W y          sample  x = A3^-1 (W y + s_ref z + sqrt(s_ref) W^1/2 w2)   [+ sigma w3 with noisy=True]

g and w come from mgp_gmrf_noise (one row-parallel pass over the CSR, noise regenerated from a counter-based generator);
the applies and solves are the library's own (Descriptor.apply, cg_solve).  Column j of a call is the sample of global
index offset + j whatever the batch size: every sample is a function of (seed, its index) alone.  Streams: tag 0 node
noise w, tag 1 edge noise (inside g), tag 2 w2, tag 3 w3.

Marginal variances (posterior_variance): diag of the posterior covariance from the same draws, var_i = s / d_i +
E[(delta_i - p_i / d_i)^2] with delta = A3^-1 p, p the perturbed right-hand side without the targets, d = diag(A3) exact
(mgp_operator_diag_exact); the moments are summed in float64 by mgp_row_moments.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .graph import require_no_self_edges

CHUNK = 256          # columns per noise launch / solve (the operator and CG paths take at most 256)
NODE_TAGS = (0, 2, 3)
# Form-3 solves run Jacobi-preconditioned CG: on the 60k manifold_784 graph (nu = 2, noise 1e-2, one column, tol 1e-5) it
# takes 20 -> 9 iterations at 50 % observed and 49 -> 23 at 10 % (0.34 -> 0.19 ms, 0.75 -> 0.39 ms), and nothing at 100 %
# (3 iterations either way; docs/kernels/sampling.md).  The form-2 path keeps the library default.
OBSERVED_JACOBI = [True]


def draw_seed():
    """A 63-bit seed from torch's default CPU generator (torch.manual_seed governs it)."""
    return int(torch.randint(0, 2 ** 63 - 1, (), dtype=torch.int64))


def _seed(seed):
    if seed is None:
        return draw_seed()
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be an int in [0, 2^64) or None, got %r" % (seed,))
    return seed


def _count(S, name="S"):
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError("%s must be a positive int, got %r" % (name, S))
    return S


def gmrf_noise(data, S, seed, offset=0, node_coef=1.0, tag=0, edges=False):
    """node_coef w_tag (+ E w_edge with edges=True) as [n, S] float32 on the graph's device: column j holds global sample
    index offset + j.  data: graph.LaplacianData (the natural-order CSR and sqrt(D))."""
    S = _count(S)
    seed = _seed(seed)
    if isinstance(offset, bool) or not isinstance(offset, int) or offset < 0:
        raise ValueError("offset must be a non-negative int, got %r" % (offset,))
    if tag not in NODE_TAGS:
        raise ValueError("tag must be one of %s (tag 1 is the edge stream), got %r" % (NODE_TAGS, tag))
    g = data.graph
    if edges:
        # the factor G = [sqrt(tau) I | E] is that of diag - S - S^T over edges between two nodes
        require_no_self_edges(g, "the edge factor of the GMRF noise (samples at odd nu)")
    csr = _lib.csr_struct(g.n, g.rowptr, g.col, data.vals, data.diag, lanes=g.spmv_lanes)
    Y = torch.empty(g.n, S, dtype=torch.float32, device=g.device)
    check(lib().mgp_gmrf_noise(ctypes.byref(csr), ptr(data.dsqrt), float(node_coef), int(tag), int(bool(edges)),
                               ctypes.c_uint64(seed), int(offset), S, ptr(Y), stream()), "mgp_gmrf_noise")
    return Y


def _check_desc(desc):
    """Form-0 precision descriptors without masks: pre = post = None (symmetric) or both sqrt(D) (random walk)."""
    if desc is None or int(desc.form) != 0 or getattr(desc, "noise", 0.0):
        raise NotImplementedError("sampling needs a form-0 precision descriptor (no noise wrapper)")
    if int(desc.nu) < 1:
        raise NotImplementedError("sampling needs an integer nu >= 1")
    if desc.pre is None and desc.post is None:
        return None
    sq = getattr(desc.data, "dsqrt", None)
    if (sq is None or desc.pre is None or desc.post is None or desc.pre.data_ptr() != sq.data_ptr()
            or desc.post.data_ptr() != sq.data_ptr()):
        raise NotImplementedError("sampling of masked (Schur-complement) descriptors is not supported")
    return sq


def _check_draws(desc):
    """_check_desc for a caller that draws z ~ N(0, Q2): at odd nu that needs the edge factor, refused on a graph with self
    edges here, ahead of everything else, as gmrf_noise refuses it."""
    P = _check_desc(desc)
    if int(desc.nu) % 2:
        require_no_self_edges(desc.data.graph, "the edge factor of the GMRF noise (samples at odd nu)")
    return P


def _tau(desc):
    return 2.0 * int(desc.nu) / (float(desc.kappa) ** 2)


def _power(desc, k, post=None, scale=1.0):
    """Descriptor of scale diag(post) A^k: nu = k at the length scale that keeps tau = 2 nu / kappa^2."""
    return desc.with_(nu=int(k), kappa=float(desc.kappa) * math.sqrt(k / int(desc.nu)), scale=float(scale), pre=None,
                      post=post, form=0, noise=0.0)


def _base_noise(desc, C, seed, offset):
    """(noise, k): g = G w_full for odd nu (k = (nu - 1) / 2), w for even nu (k = nu / 2); z = sqrt(scale) P A^k noise."""
    nu = int(desc.nu)
    if nu % 2:
        return gmrf_noise(desc.data, C, seed, offset, node_coef=math.sqrt(_tau(desc)), tag=0, edges=True), (nu - 1) // 2
    return gmrf_noise(desc.data, C, seed, offset, node_coef=1.0, tag=0, edges=False), nu // 2


def _precision_chunk(desc, P, C, seed, offset):
    noise, k = _base_noise(desc, C, seed, offset)
    rs = math.sqrt(float(desc.scale))
    if k == 0:
        return noise * (rs if P is None else rs * P.view(-1, 1))
    return _power(desc, k, post=P, scale=rs).apply(noise)


def _solve_kw(tol, refine, max_iter):
    kw = dict(tol=float(tol), stop_mode=1, max_iter=int(max_iter))
    if refine:
        kw["refine"] = int(refine)
    return kw


def precision_samples(desc, S, seed=None):
    """z ~ N(0, Q2): [S, n] float32."""
    P = _check_draws(desc)
    S, seed = _count(S), _seed(seed)
    out = torch.empty(S, desc.n, dtype=torch.float32, device=desc.data.graph.device)
    with torch.no_grad():
        for c0 in range(0, S, CHUNK):
            C = min(CHUNK, S - c0)
            out[c0:c0 + C] = _precision_chunk(desc, P, C, seed, c0).t()
    return out


def prior_samples(desc, S, seed=None, tol=1e-5, refine=0, max_iter=5000):
    """f ~ N(0, Q2^-1): [S, n] float32 (CG solves with A^k to `tol`, true relative residual per column)."""
    from .solvers import cg_solve
    P = _check_draws(desc)
    S, seed = _count(S), _seed(seed)
    nu = int(desc.nu)
    k = (nu + 1) // 2 if nu % 2 else nu // 2
    dk = _power(desc, k)
    coef = 1.0 / math.sqrt(float(desc.scale))
    pinv = None if P is None else desc.data.dinvsqrt.view(-1, 1)
    kw = _solve_kw(tol, refine, max_iter)
    out = torch.empty(S, desc.n, dtype=torch.float32, device=desc.data.graph.device)
    with torch.no_grad():
        for c0 in range(0, S, CHUNK):
            C = min(CHUNK, S - c0)
            noise, _ = _base_noise(desc, C, seed, c0)
            X = cg_solve(dk, noise, **kw)[0]
            X = X * coef if pinv is None else X * (pinv * coef)
            out[c0:c0 + C] = X.t()
    return out


def _targets(desc, y):
    _lib.require_device(y)
    y = y.reshape(-1)
    if y.shape[0] != desc.n:
        raise ValueError("y has %d entries, the graph %d nodes" % (y.shape[0], desc.n))
    return _lib.f32c(y).view(-1, 1)


class _Observation:
    """Form-3 conditioning (docs/kernels/sampling.md): s_ref, w [n, 1] and the noise standard deviation sigma [n, 1], all on
    the graph's device; obs [n, 1] bool."""

    def __init__(self, s_ref, w, sigma, obs):
        self.s_ref, self.w, self.sigma, self.obs = s_ref, w, sigma, obs

    def descriptor(self, desc):
        return desc.with_(form=3, noise=self.s_ref, obs_w=self.w.view(-1))

    def weighted_targets(self, y):
        """W y with the entries of unobserved nodes (which may be NaN) never read into the product."""
        return torch.where(self.obs, y, torch.zeros((), dtype=y.dtype, device=y.device)) * self.w


def _observation(desc, noise, observed):
    """None when the call is today's form-2 system (a python-float noise, every node observed); else the _Observation of
    form 3.  Raises ValueError for wrong lengths, non-positive / non-finite noise and an empty observed set."""
    n = desc.n
    dev = desc.data.graph.device
    if observed is not None:
        if not torch.is_tensor(observed) or observed.dtype != torch.bool:
            raise ValueError("observed must be a bool tensor [n]")
        if observed.dim() != 1 or observed.shape[0] != n:
            raise ValueError("observed has shape %s, the graph %d nodes" % (tuple(observed.shape), n))
        observed = observed.to(dev)
        if not bool(observed.any()):
            raise ValueError("observed selects no node")
    if torch.is_tensor(noise) and noise.numel() != 1:
        if noise.dim() != 1 or noise.shape[0] != n:
            raise ValueError("noise has shape %s: a float or a tensor [n] of per-node variances (n = %d)"
                             % (tuple(noise.shape), n))
        var = noise.to(device=dev, dtype=torch.float64)
        if not bool((torch.isfinite(var) & (var > 0)).all()):
            raise ValueError("per-node noise variances must be finite and positive at every node")
    else:
        # one noise (a float, or a tensor of one element such as likelihood.noise): with every node observed, today's path
        # and its checks exactly
        s = float(noise)
        if not s > 0.0:
            raise ValueError("noise must be positive, got %r" % (noise,))
        if observed is None or bool(observed.all()):
            return None
        if not math.isfinite(s):
            raise ValueError("noise must be finite when conditioning on a subset of nodes, got %r" % (noise,))
        var = torch.full((n,), s, dtype=torch.float64, device=dev)
    obs = torch.ones(n, dtype=torch.bool, device=dev) if observed is None else observed
    s_ref = float(var[obs].min())
    w = torch.where(obs, s_ref / var, torch.zeros((), dtype=torch.float64, device=dev))
    return _Observation(s_ref, w.float().view(-1, 1).contiguous(), var.sqrt().float().view(-1, 1), obs.view(-1, 1))


def _observed_rhs(desc, P, ob, yv, C, seed, offset):
    """W y + s_ref z + sqrt(s_ref) W^1/2 w2 (columns offset .. offset + C - 1)."""
    s = ob.s_ref
    z = _precision_chunk(desc, P, C, seed, offset)
    rhs = gmrf_noise(desc.data, C, seed, offset, node_coef=1.0, tag=2)
    rhs *= (s * ob.w).sqrt()
    rhs += s * z
    rhs += ob.weighted_targets(yv)
    return rhs


def posterior_rhs(desc, y, noise, C, seed, offset=0, observed=None):
    """y + s z + sqrt(s) w2 for the columns offset .. offset + C - 1 (the perturbed right-hand side of posterior_samples).
    With observed= or a per-node noise [n]: W y + s_ref z + sqrt(s_ref) W^1/2 w2, the right-hand side of form 3."""
    P = _check_draws(desc)
    one = observed is None and not (torch.is_tensor(noise) and noise.numel() != 1)
    ob = None if one else _observation(desc, noise, observed)         # (one noise, every node: unchecked, as before)
    if ob is not None:
        return _observed_rhs(desc, P, ob, _targets(desc, y), C, seed, offset)
    s = float(noise)
    z = _precision_chunk(desc, P, C, seed, offset)
    rhs = gmrf_noise(desc.data, C, seed, offset, node_coef=math.sqrt(s), tag=2)
    rhs += s * z
    rhs += _targets(desc, y)
    return rhs


def posterior_samples(desc, y, noise, S, seed=None, noisy=False, tol=1e-5, refine=0, max_iter=5000, observed=None):
    """f | y ~ N((I + s Q2)^-1 y, (Q2 + I/s)^-1) by perturb-and-MAP, s = noise: [S, n] float32.  noisy=True: samples of
    y* = f + eps (adds sqrt(s) w3).
    observed (bool [n]) and / or noise as a tensor [n] of per-node variances: f | y_observed ~ N(A3^-1 W y, (Q2 + W / s_ref)^-1)
    at every node (form 3); targets at unobserved nodes are not read (NaN allowed); noisy=True adds sigma_i w3 at every node."""
    from .solvers import cg_solve
    P = _check_draws(desc)
    S, seed = _count(S), _seed(seed)
    ob = _observation(desc, noise, observed)
    kw = _solve_kw(tol, refine, max_iter)
    out = torch.empty(S, desc.n, dtype=torch.float32, device=desc.data.graph.device)
    if ob is not None:
        kw["jacobi"] = OBSERVED_JACOBI[0]
        d3 = ob.descriptor(desc)
        with torch.no_grad():
            yv = _targets(desc, y)
            for c0 in range(0, S, CHUNK):
                C = min(CHUNK, S - c0)
                X = cg_solve(d3, _observed_rhs(desc, P, ob, yv, C, seed, c0), **kw)[0]
                if noisy:
                    X = X + gmrf_noise(desc.data, C, seed, c0, node_coef=1.0, tag=3) * ob.sigma
                out[c0:c0 + C] = X.t()
        return out
    s = float(noise)
    d2 = desc.with_(form=2, noise=s)
    with torch.no_grad():
        yv = _targets(desc, y)
        for c0 in range(0, S, CHUNK):
            C = min(CHUNK, S - c0)
            X = cg_solve(d2, posterior_rhs(desc, yv, s, C, seed, c0), **kw)[0]
            if noisy:
                X = X + gmrf_noise(desc.data, C, seed, c0, node_coef=math.sqrt(s), tag=3)
            out[c0:c0 + C] = X.t()
    return out


def posterior_mean(desc, y, noise, tol=1e-5, refine=0, max_iter=5000, observed=None):
    """(I + s Q2)^-1 y: [n] float32 (the precision-form posterior mean at the graph nodes).  observed (bool [n]) and / or
    noise as a tensor [n] of per-node variances: (W + s_ref Q2)^-1 W y (form 3), targets at unobserved nodes not read."""
    from .solvers import cg_solve
    _check_desc(desc)
    ob = _observation(desc, noise, observed)
    with torch.no_grad():
        if ob is not None:
            rhs = ob.weighted_targets(_targets(desc, y))
            return cg_solve(ob.descriptor(desc), rhs, jacobi=OBSERVED_JACOBI[0], **_solve_kw(tol, refine, max_iter))[0].view(-1)
        s = float(noise)
        return cg_solve(desc.with_(form=2, noise=s), _targets(desc, y), **_solve_kw(tol, refine, max_iter))[0].view(-1)


# ---------------------------------------------------------------------------------------------- marginal variances
RB_MAX_NU = 3        # mgp_operator_diag_exact: the exact diagonal of A3 exists for nu <= 3


def operator_diag_exact(desc):
    """The exact diagonal of a form 0 / 2 / 3 descriptor (nu <= 3): [n] float64 on the graph's device.  ValueError on a graph
    with self edges (the kernel reads col == row as padding)."""
    require_no_self_edges(desc.data.graph, "the exact operator diagonal (Rao-Blackwell variances)")
    op = desc.struct()
    dev = desc.data.graph.device
    d = torch.empty(desc.n, dtype=torch.float64, device=dev)
    wb = lib().mgp_operator_diag_exact_workspace_bytes(ctypes.byref(op))
    work = _lib.workspace(wb, "diag_exact", dev) if wb else None
    check(lib().mgp_operator_diag_exact(ctypes.byref(op), ptr(d), ptr(work), wb, stream()), "mgp_operator_diag_exact")
    return d


def row_moments(acc, U, V=None, rdiag=None, Pm=None):
    """acc [n, 2] float64 += (sum_c u v, sum_c (u v)^2) over the columns of U [n, C] float32, u = U - Pm rdiag, v likewise
    from V (None: v = u); C <= 256 (mgp_row_moments)."""
    n, C = U.shape
    check(lib().mgp_row_moments(ptr(U), ptr(V), ptr(rdiag), ptr(Pm), int(n), int(C), ptr(acc), stream()), "mgp_row_moments")
    return acc


def _perturbation(desc, P, ob, s, C, seed, offset):
    """p = s z + sqrt(s) W^1/2 w2 (columns offset .. offset + C - 1): the right-hand side of posterior_samples without the
    targets; s = s_ref and W = diag(ob.w) for form 3, W = I for form 2 (ob None)."""
    z = _precision_chunk(desc, P, C, seed, offset)
    if ob is None:
        p = gmrf_noise(desc.data, C, seed, offset, node_coef=math.sqrt(s), tag=2)
    else:
        p = gmrf_noise(desc.data, C, seed, offset, node_coef=1.0, tag=2)
        p *= (s * ob.w).sqrt()
    p += s * z
    return p


def posterior_variance(desc, noise, S=64, seed=None, observed=None, method="rao-blackwell", noisy=False, tol=1e-6, refine=1,
                       max_iter=5000):
    """(var, se): the marginal posterior variance diag((Q2 + W / s)^-1) at every node and the standard error of the estimate,
    float64 [n] each, from S perturb-and-MAP draws delta = A3^-1 p around the mean (the targets do not enter).
    method "rao-blackwell" (nu <= 3): var_i = s / d_i + mean_s (delta_is - p_is / d_i)^2 with d = diag(A3) exact -- the
    variance of node i given all others plus the variance of its conditional mean; unbiased, and never more variable than
    "samples", the plain mean_s delta_is^2 (any nu).  se_i = sqrt((mean e^4 - (mean e^2)^2) / S) of the averaged term.
    noise / observed as in posterior_samples; noisy=True adds the noise variance sigma_i^2 (the variance of y*)."""
    from .solvers import cg_solve
    P = _check_draws(desc)
    S, seed = _count(S), _seed(seed)
    if method not in ("rao-blackwell", "samples"):
        raise ValueError("method must be 'rao-blackwell' or 'samples', got %r" % (method,))
    rb = method == "rao-blackwell"
    if rb and int(desc.nu) <= RB_MAX_NU:
        require_no_self_edges(desc.data.graph, "the exact operator diagonal (Rao-Blackwell variances)")
    ob = _observation(desc, noise, observed)
    if rb and int(desc.nu) > RB_MAX_NU:
        raise NotImplementedError("method='rao-blackwell' needs the exact diagonal of the system, which exists for nu <= %d "
                                  "(nu = %d): use method='samples'" % (RB_MAX_NU, int(desc.nu)))
    kw = _solve_kw(tol, refine, max_iter)
    if ob is not None:
        kw["jacobi"] = OBSERVED_JACOBI[0]
        s, dsys = ob.s_ref, ob.descriptor(desc)
    else:
        s = float(noise)
        dsys = desc.with_(form=2, noise=s)
    dev = desc.data.graph.device
    acc = torch.zeros(desc.n, 2, dtype=torch.float64, device=dev)
    with torch.no_grad():
        rdiag = operator_diag_exact(dsys).reciprocal() if rb else None
        for c0 in range(0, S, CHUNK):
            C = min(CHUNK, S - c0)
            p = _perturbation(desc, P, ob, s, C, seed, c0)
            row_moments(acc, _lib.f32c(cg_solve(dsys, p, **kw)[0]), None, rdiag, p if rb else None)
        m2, m4 = acc[:, 0] / S, acc[:, 1] / S
        var = m2 + s * rdiag if rb else m2
        se = ((m4 - m2 * m2).clamp_min(0.0) / S).sqrt()
        if noisy:
            per_node = torch.is_tensor(noise) and noise.numel() != 1
            var = var + (noise.to(device=dev, dtype=torch.float64) if per_node else float(noise))
    return var, se


def posterior_stddev(desc, noise, S=64, seed=None, observed=None, method="rao-blackwell", noisy=False, tol=1e-6, refine=1,
                     max_iter=5000):
    """The marginal posterior standard deviation at every node: sqrt of posterior_variance(...)[0], float64 [n]."""
    return posterior_variance(desc, noise, S, seed, observed, method, noisy, tol, refine, max_iter)[0].clamp_min(0).sqrt()
