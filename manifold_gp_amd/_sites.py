"""The host side the per-node wrappers share (csrc/laplace.hip: site_kernel, evidence_kernel): coercion, the checks with their
messages, the outputs and the workspace.  The family's own validation and its one ctypes call stay with each wrapper."""
import torch

from . import _lib


def _int(v, name):
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError("%s must be an int, got %r" % (name, v))
    return v


def _real(v, name):
    """float(v) of a real scalar: a Python or numpy number, or a tensor of one element"""
    if isinstance(v, (bool, str)) or (torch.is_tensor(v) and (v.numel() != 1 or v.dtype == torch.bool)):
        raise ValueError("%s must be a real scalar, got %r" % (name, v))
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a real scalar (a number or a tensor of one element), got %s" % (name, type(v).__name__))


def _node_vector(t, n, name):
    if not torch.is_tensor(t) or t.numel() != n or t.dtype == torch.bool:
        raise ValueError("%s must be a tensor of %d values, got %s" % (name, n, tuple(t.shape) if torch.is_tensor(t) else type(t)))
    return t.reshape(-1).to(torch.float64)


def threshold(k, n, name, last):
    """The threshold of a predict_exceedance: an int or an integer tensor of n values, all in 0 .. last.  Returns (the thresholds
    as int64 [n] or None for the one int, the largest)."""
    if torch.is_tensor(k):
        if k.dtype == torch.bool or k.is_floating_point() or k.is_complex() or k.numel() != n:
            raise ValueError("%s must be an int or an integer tensor of %d values" % (name, n))
        thr = k.reshape(-1).to(torch.int64)
        low, top = int(thr.min()), int(thr.max())
    else:
        low = top = _int(k, name)
        thr = None
    if low < 0 or top > last:
        raise ValueError("%s must lie in 0 .. %d, got %d .. %d" % (name, last, low, top))
    _lib.require_device(thr)
    return thr, top


def learning_args(steps, lr, variance):
    """The checks learn_dispersion and learn_cutpoints share; returns steps"""
    steps = _int(steps, "steps")
    if steps < 1 or not float(lr) > 0.0:
        raise ValueError("steps must be >= 1 and lr positive, got %r and %r" % (steps, lr))
    if variance is not None and not callable(variance):
        raise ValueError("variance must be None or a callable fit -> tensor [n]")
    return steps


def check_mask(observed, n, name="observed"):
    """The mask of a fit's data: None (every node) or a bool tensor [n] that selects a node; returned as it came"""
    if observed is None:
        return None
    if not torch.is_tensor(observed) or observed.dtype != torch.bool:
        raise ValueError("%s must be a bool tensor [n]" % name)
    if observed.dim() != 1 or observed.shape[0] != n:
        raise ValueError("%s has shape %s, the graph %d nodes" % (name, tuple(observed.shape), n))
    if not bool(observed.any()):
        raise ValueError("%s selects no node" % name)
    return observed


def picker(observed):
    """t -> the entries of t the mask selects (None: all of them), on t's device"""
    return (lambda t: t) if observed is None else (lambda t: t[observed.to(t.device)])


def newton_args(f, qf, required, optional, observed, tag, workspace_bytes):
    """The arguments of a Newton-stage entry point.  f [n] and the `required` (name, tensor) pairs as contiguous float32, qf and
    the `optional` pairs likewise (None stays), observed bool [n] or None; every one of length n.  Returns (f, qf, arrays,
    observed, n, w, rhs, sums, work): arrays the required then the optional tensors, w, rhs fresh float32 [n], sums float64 [4],
    work the `tag` workspace of workspace_bytes(n) bytes."""
    _lib.require_device(f, qf, *(t for _, t in tuple(required) + tuple(optional)), observed)
    f = _lib.f32c(f.reshape(-1))
    arrays = [(name, _lib.f32c(t.reshape(-1))) for name, t in required]
    arrays += [(name, None if t is None else _lib.f32c(t.reshape(-1))) for name, t in optional]
    n = f.shape[0]
    qf = None if qf is None else _lib.f32c(qf.reshape(-1))
    if observed is not None:
        if observed.dtype != torch.bool:
            raise ValueError("observed must be a bool tensor [n]")
        observed = observed.reshape(-1).contiguous()
    for name, t in [("qf", qf)] + arrays + [("observed", observed)]:
        if t is not None and t.shape[0] != n:
            raise ValueError("%s has %d entries, f %d" % (name, t.shape[0], n))
    w, rhs = torch.empty_like(f), torch.empty_like(f)
    sums = torch.empty(4, dtype=torch.float64, device=f.device)
    work = _lib.workspace(workspace_bytes(n), tag, f.device)
    return f, qf, [t for _, t in arrays], observed, n, w, rhs, sums, work


def check_evidence_args(f, required, optional, observed, variance, h_floor, extra=()):
    """The host-side checks the evidence kernels share: f and the `required` (name, tensor) pairs tensors of one length n >= 1,
    observed bool [n] or None, the `optional` pairs, variance and the `extra` pairs [n] or None, h_floor >= 0.  Returns n."""
    if not float(h_floor) >= 0.0:
        raise ValueError("h_floor must be >= 0, got %r" % (h_floor,))
    for name, t in (("f", f),) + tuple(required):
        if not torch.is_tensor(t):
            raise ValueError("%s must be a tensor [n]" % name)
    n = f.numel()
    if observed is not None and (not torch.is_tensor(observed) or observed.dtype != torch.bool):
        raise ValueError("observed must be a bool tensor [n]")
    for name, t in tuple(required) + tuple(optional) + (("observed", observed), ("variance", variance)) + tuple(extra):
        if t is not None and (not torch.is_tensor(t) or t.numel() != n):
            raise ValueError("%s has %s entries, f %d" % (name, t.numel() if torch.is_tensor(t) else type(t), n))
    if n < 1:
        raise ValueError("f has no entries")
    return n


def evidence_args(f, required, optional, observed, variance, h_floor, workspace_bytes):
    """The arguments of an evidence-stage entry point after check_evidence_args: f and the arrays as contiguous float32, variance
    as float64.  Returns (f, arrays, observed, variance, n, root_h, corr, sums, work): root_h fresh float32 [n], corr likewise or
    None without a variance, sums float64 [4], work the "evidence_site" workspace of workspace_bytes(n) bytes."""
    n = check_evidence_args(f, required, optional, observed, variance, h_floor)
    arrays = [t for _, t in tuple(required) + tuple(optional)]
    _lib.require_device(f, *arrays, observed, variance)
    f = _lib.f32c(f.reshape(-1))
    arrays = [None if t is None else _lib.f32c(t.reshape(-1)) for t in arrays]
    observed = None if observed is None else observed.reshape(-1).contiguous()
    variance = None if variance is None else variance.reshape(-1).to(torch.float64).contiguous()
    root_h = torch.empty_like(f)
    corr = None if variance is None else torch.empty_like(f)
    sums = torch.empty(4, dtype=torch.float64, device=f.device)
    work = _lib.workspace(workspace_bytes(n), "evidence_site", f.device)
    return f, arrays, observed, variance, n, root_h, corr, sums, work
