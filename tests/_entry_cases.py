"""One case per entry point of the C ABI for the memory contract (tests/test_gpu_memory_contract.py, docs/memory_contract.md).

CASES is keyed by the names of manifold_gp_amd._lib.SIGNATURES.  A case is a function (carve, shape) -> _guarded.Call: it carves
every array the call sees from the arena -- carve(name, dtype, numel, role, init, floor) with role "in" / "inout" / "out" / "work" --
builds the ctypes arguments on the views' pointers and says what the documented extent of each output is.  The same function is run
once with a recording carve (sizes only) and once per arena.  Inputs are built the way the entry point's own GPU test builds them;
hand-built rings give the tiny CSRs.

A case may run a sequence (plan create / solve / rebind / destroy, begin / step / end): COVERED_BY names the entry points that are
exercised inside another one's case.  EXEMPT names those that launch no device work of their own on caller memory, each with its
category.  PENDING names those that do and have no case yet (none today).  tests/test_guarded_cpu.py keeps the four sets a
partition of SIGNATURES, so a new entry point cannot be added without landing in one of them.

The same cases run on a side stream behind pending work (tests/test_gpu_stream_order.py, docs/stream_contract.md): every case takes
its stream from _stream() when it is built or run, and _sync() -- the device sync between the steps of a sequence and behind every
call -- runs SYNC_HOOK behind the sync when one is set, which is where that run re-arms the arena.
"""
import contextlib
import ctypes
import re

import numpy as np
import torch

from manifold_gp_amd import _lib
from _guarded import Call

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
P = _lib.ptr


def _stream():
    return _lib.stream() if torch.cuda.is_available() else ctypes.c_void_p(0)


SYNC_HOOK = None          # set by _guarded.sync_hook for the length of a side-stream run (tests/test_gpu_stream_order.py), else None


def _sync():
    """The device sync between the steps of a sequence and behind a call; SYNC_HOOK, when set, runs right behind it."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if SYNC_HOOK is not None:
        SYNC_HOOK()


def _rng(shape, salt=0):
    return np.random.default_rng(1000003 * salt + sum((i + 1) * int(v) for i, v in enumerate(shape.values()) if isinstance(v, int)))


def _call(fn, args, query=0, work_pos=None, **kw):
    """A Call around one library call: args is the ctypes argument list; work_pos the index of work_bytes in it."""
    def run(work_bytes):
        a = list(args)
        if work_bytes is not None:
            a[work_pos] = work_bytes
        rc = getattr(_lib.lib(), fn)(*a)
        _sync()
        return rc, {}
    return Call(run, query=query, **kw)


# ====================================================================================================== per-node (site) inputs
def _site_inputs(carve, shape, rng, names):
    """Carves the per-node inputs the site kernels share, by name; returns {name: view}.  obs keeps node 0 observed."""
    n = shape["n"]
    cat = rng.integers(0, 4, n)
    cuts = np.array([-np.inf, -1.0, 0.5, 2.0, np.inf], np.float32)
    counts = rng.poisson(3.0, n).astype(np.float32)
    obs = (rng.random(n) > 0.3).astype(np.uint8)
    obs[0] = 1
    gen = {
        "f": lambda: (F32, rng.normal(0, 1.5, n)), "qf": lambda: (F32, rng.normal(0, 1.0, n)),
        "y01": lambda: (F32, (rng.random(n) > 0.5).astype(np.float32)), "counts": lambda: (F32, counts),
        "trials": lambda: (F32, counts + rng.integers(0, 5, n)), "logexp": lambda: (F32, rng.normal(0, 0.3, n)),
        "obs": lambda: (U8, obs), "var": lambda: (F64, rng.uniform(0.1, 2.0, n)), "u": lambda: (F64, rng.normal(0, 1.0, n)),
        "lo": lambda: (F32, cuts[cat]), "hi": lambda: (F32, cuts[cat + 1]), "cat": lambda: (U8, cat.astype(np.uint8)),
        "eta": lambda: (F64, rng.normal(0.5, 1.0, n)), "mean32": lambda: (F32, rng.normal(0, 1.5, n)),
    }
    out = {}
    for name in names:
        dtype, val = gen[name]()
        out[name] = carve(name, dtype, n, "in", val)
    return out


def _newton(fn, query_fn, in_names, scalars_after_n):
    """f, qf, <in_names>, obs, n, <scalars>, w, rhs, sums, work, work_bytes, stream."""
    def case(carve, shape):
        n = shape["n"]
        a = _site_inputs(carve, shape, _rng(shape), ["f", "qf"] + in_names + ["obs"])
        w, rhs = carve("w", F32, n, "out"), carve("rhs", F32, n, "out")
        sums = carve("sums", F64, 4, "out")
        q = getattr(_lib.lib(), query_fn)(n)
        work = carve("work", U8, q, "work", floor=8)
        scal = shape.get("scalars", scalars_after_n)
        args = [P(a["f"]), P(a["qf"])] + [P(a[k]) for k in in_names] + [P(a["obs"]), n] + list(scal) + \
               [P(w), P(rhs), P(sums), P(work), q, _stream()]
        return _call(fn, args, q, len(args) - 2)
    return case


def _evidence(fn, query_fn, in_names, scalars_after_n):
    """f, <in_names>, obs, var, n, <scalars>, root_h, corr, sums, work, work_bytes, stream."""
    def case(carve, shape):
        n = shape["n"]
        a = _site_inputs(carve, shape, _rng(shape), ["f"] + in_names + ["obs", "var"])
        root_h, corr = carve("root_h", F32, n, "out"), carve("corr", F32, n, "out")
        sums = carve("sums", F64, 4, "out")
        q = getattr(_lib.lib(), query_fn)(n)
        work = carve("work", U8, q, "work", floor=8)
        scal = shape.get("scalars", scalars_after_n)
        args = [P(a["f"])] + [P(a[k]) for k in in_names] + [P(a["obs"]), P(a["var"]), n] + list(scal) + \
               [P(root_h), P(corr), P(sums), P(work), q, _stream()]
        return _call(fn, args, q, len(args) - 2)
    return case


def case_nb_dispersion_sums(carve, shape):
    n = shape["n"]
    a = _site_inputs(carve, shape, _rng(shape), ["f", "counts", "logexp", "obs", "var", "u"])
    out = carve("out", F64, 3, "out")                       # the caller is promised three entries
    q = _lib.lib().mgp_nb_dispersion_sums_workspace_bytes(n)
    work = carve("work", U8, q, "work", floor=8)
    args = [P(a["f"]), P(a["counts"]), P(a["logexp"]), P(a["obs"]), P(a["var"]), P(a["u"]), n, 0.2, 3.5, 1e-6, P(out), P(work), q,
            _stream()]
    return _call("mgp_nb_dispersion_sums", args, q, 12)


def case_ordinal_cut_sums(carve, shape):
    n, K = shape["n"], shape["K"]
    rng = _rng(shape)
    cutv = np.concatenate([[-np.inf], np.linspace(-2.0, 2.0, K - 1), [np.inf]]).astype(np.float32)
    cat = rng.integers(0, K, n)
    obs = (rng.random(n) > 0.3).astype(np.uint8)
    obs[0] = 1
    f = carve("f", F32, n, "in", rng.normal(0, 1.5, n))
    lo, hi = carve("lo", F32, n, "in", cutv[cat]), carve("hi", F32, n, "in", cutv[cat + 1])
    catv, obsv = carve("cat", U8, n, "in", cat), carve("obs", U8, n, "in", obs)
    var, u = carve("var", F64, n, "in", rng.uniform(0.1, 2.0, n)), carve("u", F64, n, "in", rng.normal(0, 1, n))
    out = carve("out", F64, 3 * (K - 1), "out")
    q = _lib.lib().mgp_ordinal_cut_sums_workspace_bytes(n, K)
    work = carve("work", U8, q, "work", floor=8)
    args = [P(f), P(lo), P(hi), P(catv), P(obsv), P(var), P(u), n, K, 1e-6, P(out), P(work), q, _stream()]
    return _call("mgp_ordinal_cut_sums", args, q, 12)


def _softmax_pi(rng, n, C, zero_rows=True):
    f = rng.normal(0, 1.5, (n, C))
    e = np.exp(f - f.max(1, keepdims=True))
    pi = (e / e.sum(1, keepdims=True)).astype(np.float32)
    if zero_rows and n > 2:
        pi[rng.random(n) < 0.2] = 0.0                       # unobserved rows
    return pi


def case_softmax_site(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    obs = (rng.random(n) > 0.3).astype(np.uint8)
    obs[0] = 1
    f, qf = carve("f", F32, n * C, "in", rng.normal(0, 1.5, n * C)), carve("qf", F32, n * C, "in", rng.normal(0, 1, n * C))
    labels, obsv = carve("labels", I32, n, "in", rng.integers(0, C, n)), carve("obs", U8, n, "in", obs)
    pi, rhs = carve("pi", F32, n * C, "out"), carve("rhs", F32, n * C, "out")
    sums = carve("sums", F64, 4, "out")
    q = _lib.lib().mgp_softmax_site_workspace_bytes(n, C)
    work = carve("work", U8, q, "work", floor=8)
    args = [P(f), P(qf), P(labels), P(obsv), n, C, P(pi), P(rhs), P(sums), P(work), q, _stream()]
    return _call("mgp_softmax_site", args, q, 10)


def case_softmax_hessian_add(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    pi = carve("pi", F32, n * C, "in", _softmax_pi(rng, n, C))
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "inout", rng.normal(0, 1, n * C))
    return _call("mgp_softmax_hessian_add", [P(pi), P(X), n, C, P(Y), _stream()])


def case_softmax_hessian_add_block(carve, shape):
    n, C, S = shape["n"], shape["C"], shape["S"]
    rng = _rng(shape)
    pi = carve("pi", F32, n * C, "in", _softmax_pi(rng, n, C))
    X = carve("X", F32, n * S * C, "in", rng.normal(0, 1, n * S * C))
    Y = carve("Y", F32, n * S * C, "inout", rng.normal(0, 1, n * S * C))
    sums = carve("sums", F64, 2 * S, "out")
    q = _lib.lib().mgp_softmax_hessian_add_block_workspace_bytes(n, C, S)
    work = carve("work", U8, q, "work", floor=16)
    args = [P(pi), P(X), n, C, S, P(Y), P(sums), P(work), q, _stream()]
    return _call("mgp_softmax_hessian_add_block", args, q, 8)


def case_softmax_root_apply(carve, shape):
    n, C, S, tr = shape["n"], shape["C"], shape["S"], shape["transpose"]
    rng = _rng(shape)
    cs, ss = (S, 1) if shape["layout"] == "ncs" else (1, C)
    pi = carve("pi", F32, n * C, "in", _softmax_pi(rng, n, C))
    V = carve("V", F32, n * C * S, "in", rng.normal(0, 1, n * C * S))
    X = carve("X", F32, n * C * S, "in", rng.normal(0, 1, n * C * S))
    out = carve("out", F32, n * C * S, "out")
    args = [P(pi), P(V), P(X) if tr else None, n, C, S, cs, ss, tr, P(out), _stream()]
    return _call("mgp_softmax_root_apply", args)


def case_softmax_curvature(carve, shape):
    n, C, S = shape["n"], shape["C"], shape["S"]
    rng = _rng(shape)
    pi = carve("pi", F32, n * C, "in", _softmax_pi(rng, n, C))
    delta = carve("delta", F32, n * S * C, "in", rng.normal(0, 1, n * S * C))
    acc = carve("acc", F64, n * C, "inout", rng.normal(0, 1, n * C))
    acc2 = carve("acc2", F64, n * C, "inout", rng.uniform(0, 1, n * C))
    return _call("mgp_softmax_curvature", [P(pi), P(delta), n, C, S, P(acc), P(acc2), _stream()])


def case_scale_rows(carve, shape):
    n, Pc = shape["n"], shape["P"]
    rng = _rng(shape)
    s = carve("s", F32, n, "in", rng.normal(0, 1, n))
    V = carve("V", F32, n * Pc, "in", rng.normal(0, 1, n * Pc))
    X = carve("X", F32, n * Pc, "in", rng.normal(0, 1, n * Pc))
    out = carve("out", F32, n * Pc, "out")
    return _call("mgp_scale_rows", [P(s), P(V), P(X) if shape["with_x"] else None, n, Pc, P(out), _stream()])


def case_row_moments(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    U = carve("U", F32, n * C, "in", rng.normal(0, 1, n * C))
    V = carve("V", F32, n * C, "in", rng.normal(0, 1, n * C))
    rdiag = carve("rdiag", F64, n, "in", rng.uniform(0.5, 2, n))
    Pm = carve("Pm", F32, n * C, "in", rng.normal(0, 1, n * C))
    acc0 = rng.uniform(0, 1, 2 * n)
    acc = carve("acc", F64, 2 * n, "inout", acc0)
    # float4 loads at C % 4 == 0 on 16-byte aligned blocks, scalar loads otherwise (header): another order of the same float64 sum.
    # The bar of test_gpu_variance.py: 1e-12 of the sum of the absolute terms (plus the state added to)
    f64 = lambda t: t.double().cpu().numpy()
    sub = f64(Pm).reshape(n, C) * f64(rdiag)[:, None]
    p = (f64(U).reshape(n, C) - sub) * (f64(V).reshape(n, C) - sub)
    tol = 1e-12 * (np.stack([np.abs(p).sum(1), (p * p).sum(1)], 1) + np.abs(acc0).reshape(n, 2))
    return _call("mgp_row_moments", [P(U), P(V), P(rdiag), P(Pm), n, C, P(acc), _stream()],
                 placement_bar=("1e-12 of the sum of the absolute terms, as test_gpu_variance.py", {"acc": tol}))


def case_bernoulli_predict(carve, shape):
    n = shape["n"]
    a = _site_inputs(carve, shape, _rng(shape), ["mean32", "var"])
    prob = carve("prob", F64, n, "out")
    return _call("mgp_bernoulli_predict", [P(a["mean32"]), P(a["var"]), n, shape["points"], P(prob), _stream()])


def case_ordinal_predict(carve, shape):
    n, K = shape["n"], shape["K"]
    a = _site_inputs(carve, shape, _rng(shape), ["eta", "var"])
    cuts = carve("cuts", F64, K - 1, "in", np.linspace(-2.0, 2.0, K - 1))
    out = carve("out", F64, n * K, "out")
    args = [P(a["eta"]), P(a["var"]), P(cuts), n, K, shape["points"], shape["log_out"], P(out), _stream()]
    return _call("mgp_ordinal_predict", args)


def case_count_predict_pmf(carve, shape):
    n, K, fam = shape["n"], shape["K"], shape["family"]
    a = _site_inputs(carve, shape, _rng(shape), ["eta", "var", "trials" if fam == 1 else "logexp"])
    out = carve("out", F64, n * K, "out")
    args = [P(a["eta"]), P(a["var"]), P(a["trials" if fam == 1 else "logexp"]), n, fam, shape["k0"], K, shape["points"], 1, P(out),
            _stream()]
    return _call("mgp_count_predict_pmf", args)


def case_count_predict_logpmf(carve, shape):
    n, fam = shape["n"], shape["family"]
    a = _site_inputs(carve, shape, _rng(shape), ["eta", "var", "trials" if fam == 1 else "logexp", "counts", "obs"])
    out = carve("out", F64, n, "out")
    args = [P(a["eta"]), P(a["var"]), P(a["trials" if fam == 1 else "logexp"]), P(a["counts"]), P(a["obs"]), n, fam, shape["points"],
            P(out), _stream()]
    return _call("mgp_count_predict_logpmf", args)


def case_nb_predict_pmf(carve, shape):
    n, K = shape["n"], shape["K"]
    a = _site_inputs(carve, shape, _rng(shape), ["eta", "var", "logexp"])
    out = carve("out", F64, n * K, "out")
    args = [P(a["eta"]), P(a["var"]), P(a["logexp"]), n, 3.5, shape["k0"], K, shape["points"], 0, P(out), _stream()]
    return _call("mgp_nb_predict_pmf", args)


def case_nb_predict_logpmf(carve, shape):
    n = shape["n"]
    a = _site_inputs(carve, shape, _rng(shape), ["eta", "var", "logexp", "counts", "obs"])
    out = carve("out", F64, n, "out")
    args = [P(a["eta"]), P(a["var"]), P(a["logexp"]), P(a["counts"]), P(a["obs"]), n, 3.5, shape["points"], P(out), _stream()]
    return _call("mgp_nb_predict_logpmf", args)


def case_permute_rows(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    src = carve("src", F32, n * C, "in", rng.normal(0, 1, n * C))
    order = carve("order", I32, n, "in", rng.permutation(n))
    dst = carve("dst", F32, n * C, "out")
    return _call("mgp_permute_rows", [P(src), P(order), n, C, P(dst), _stream()])


# ============================================================================================================ hand-built rings
def ring_csr(n, rng):
    """The padded CSR of a ring on n >= 3 nodes as the graph builders write it: a row holds its two neighbours in ascending column
    order and two padding entries (col = own row, d2 = +inf, value 0) behind them; every row start is a multiple of MGP_PAD."""
    assert n >= 3
    i = np.arange(n)
    nb = np.sort(np.stack([(i - 1) % n, (i + 1) % n], 1), 1)
    col = np.concatenate([nb, np.stack([i, i], 1)], 1).astype(np.int32)
    ed = rng.uniform(0.05, 1.5, n).astype(np.float32)          # edge e = (e, e + 1 mod n)
    dist = np.where(nb == ((i + 1) % n)[:, None], ed[i][:, None], ed[(i - 1) % n][:, None])
    d2 = np.concatenate([dist, np.full((n, 2), np.inf)], 1).astype(np.float32)
    sv = np.concatenate([np.exp(-dist), np.zeros((n, 2))], 1).astype(np.float32)          # symmetric positive S_ij
    diag = (sv.sum(1) + 0.1).astype(np.float32)
    return dict(n=n, rowptr=(4 * np.arange(n + 1)).astype(np.int32), col=col.reshape(-1), d2=d2.reshape(-1), vals=sv.reshape(-1),
                diag=diag, nnz=4 * n)


def _carve_csr(carve, g, want=("rowptr", "col", "vals", "diag")):
    """CSR index and value arrays are read in 16-byte quads (MGP_PAD): floor 0."""
    dt = dict(rowptr=I32, col=I32, vals=F32, diag=F32, d2=F32)
    return {k: carve(k, dt[k], g[k].size, "in", g[k], floor=0 if k in ("col", "vals", "d2") else None) for k in want}


def _csr_struct(g, v):
    return _lib.csr_struct(g["n"], v["rowptr"], v["col"], v["vals"], v["diag"])


def _operator(g, v, form=2, nu=2, obs_w=None):
    op = _lib.OperatorT()
    op.L = _csr_struct(g, v)
    op.pre, op.post = None, None
    op.nu, op.kappa, op.scale, op.form, op.noise = nu, 1.0, 0.7, form, 0.1
    op.obs_w = None if obs_w is None else obs_w.data_ptr()
    return op


def case_laplacian_build(carve, shape):
    n = shape["n"]
    g = ring_csr(n, _rng(shape))
    v = _carve_csr(carve, g, ("rowptr", "col", "d2"))
    outs = [carve(k, F32, n, "out") for k in ("degree_unnorm", "degree", "diag", "dsqrt", "dinvsqrt")]
    vals = carve("vals", F32, g["nnz"], "out", floor=0)
    args = [n, P(v["rowptr"]), P(v["col"]), P(v["d2"]), 0.8, 0] + [P(t) for t in outs] + [P(vals), _stream()]
    return _call("mgp_laplacian_build", args)


def case_spmm_fused(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    csr = _csr_struct(g, v)
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C))
    pre, post = carve("pre", F32, n, "in", rng.uniform(0.5, 2, n)), carve("post", F32, n, "in", rng.uniform(0.5, 2, n))
    base, dotw = carve("base", F32, n * C, "in", rng.normal(0, 1, n * C)), carve("dotw", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "out")
    blocks = _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(csr), C)
    assert blocks > 0
    part = carve("dot_partials", F32, blocks * C, "out")
    args = [ctypes.byref(csr), P(X), C, P(Y), 0.3, 1.1, P(pre), P(post), P(base), 0.5, 0.9, P(dotw), P(part), _stream()]
    call = _call("mgp_spmm_fused", args)
    call.keep = (csr,)

    def probe(host):
        assert _lib.lib().mgp_spmm_kernel_choice(ctypes.byref(csr), C, 1, 0) == 0, "the ring CSR carries no tiles: gather kernels"
    call.probe = probe
    return call


def case_operator_apply(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    op = _operator(g, v, form=shape.get("form", 2))
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "out")
    q = _lib.lib().mgp_operator_workspace_bytes(ctypes.byref(op), C)
    work = carve("work", U8, q, "work", floor=16)
    call = _call("mgp_operator_apply", [ctypes.byref(op), P(X), C, P(Y), P(work), q, _stream()], q, 5)
    call.keep = (op,)
    return call


def case_operator_jacobi(carve, shape):
    n = shape["n"]
    g = ring_csr(n, _rng(shape))
    v = _carve_csr(carve, g)
    op = _operator(g, v)
    minv = carve("minv", F32, n, "out")
    call = _call("mgp_operator_jacobi", [ctypes.byref(op), P(minv), _stream()])
    call.keep = (op,)
    return call


def case_operator_apply_double(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    op = _operator(g, v)
    X = carve("X", F64, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F64, n * C, "out")
    q = _lib.lib().mgp_operator_apply_double_workspace_bytes(ctypes.byref(op), C)
    work = carve("work", U8, q, "work", floor=8)
    call = _call("mgp_operator_apply_double", [ctypes.byref(op), P(X), C, P(Y), P(work), q, _stream()], q, 5)
    call.keep = (op,)
    return call


def case_operator_diag_exact(carve, shape):
    n = shape["n"]
    g = ring_csr(n, _rng(shape))
    v = _carve_csr(carve, g)
    op = _operator(g, v, nu=shape["nu"])
    out = carve("diag_out", F64, n, "out")
    assert _lib.lib().mgp_operator_diag_exact_workspace_bytes(ctypes.byref(op)) == 0
    call = _call("mgp_operator_diag_exact", [ctypes.byref(op), P(out), None, 0, _stream()])
    call.keep = (op,)
    return call


def case_gmrf_noise(carve, shape):
    n, S = shape["n"], shape["S"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    csr = _csr_struct(g, v)
    dsqrt = carve("dsqrt", F32, n, "in", rng.uniform(0.5, 2, n))
    Y = carve("Y", F32, n * S, "out")
    args = [ctypes.byref(csr), P(dsqrt), 0.7, 0, 1, ctypes.c_uint64(1234), 5, S, P(Y), _stream()]
    call = _call("mgp_gmrf_noise", args)
    call.keep = (csr,)
    return call


def case_laplacian_matmul(carve, shape):
    n, C, mode = shape["n"], shape["C"], shape["mode"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    csr = _csr_struct(g, v)
    ds = rng.uniform(0.5, 2, n).astype(np.float32)
    dsqrt, dinv = carve("dsqrt", F32, n, "in", ds), carve("dinvsqrt", F32, n, "in", 1 / ds)
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "out")
    call = _call("mgp_laplacian_matmul", [ctypes.byref(csr), P(dsqrt), P(dinv), mode, P(X), C, P(Y), None, _stream()])
    call.keep = (csr,)
    return call


def case_cg_solve(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    op = _operator(g, v)
    B = carve("B", F32, n * C, "in", rng.normal(0, 1, n * C))
    X = carve("X", F32, n * C, "out")
    q = _lib.lib().mgp_cg_workspace_bytes(ctypes.byref(op), C)
    work = carve("work", U8, q, "work", floor=16)
    params = _lib.CgParamsT(1e-4, 200, 0, 1, 0, 0, 0)

    def run(work_bytes):
        iters, resid = ctypes.c_int32(-7), (ctypes.c_float * C)()
        rc = _lib.lib().mgp_cg_solve(ctypes.byref(op), P(B), C, P(X), None, ctypes.byref(params), ctypes.byref(iters), resid, P(work),
                                     q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(iters=np.int32(iters.value), resid=np.array(list(resid), np.float32)))
    return Call(run, query=q)


# ======================================================================================================= graph stages on rings
I16 = torch.int16          # the uint16 `lid` of the tile dictionaries, as manifold_gp_amd.graph holds it


def ring_coo(n, rng):
    """The ring's edge list in the reference's order (row < col, sorted, unique) with random squared distances."""
    pairs = np.unique(np.array([(min(i, (i + 1) % n), max(i, (i + 1) % n)) for i in range(n)], np.int64), axis=0)
    return pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32), rng.uniform(0.05, 1.5, len(pairs)).astype(np.float32)


def ring_tiles(g, rows):
    """Row-tile column dictionaries of a ring CSR as mgp_graph_tiles writes them (natural row order): tile_ptr, tile_cols (ascending
    distinct columns per tile), lid (position of every entry's column in its tile's list), max_cols, max_entries."""
    n, col, rowptr = g["n"], g["col"], g["rowptr"]
    tile_ptr, tile_cols, lid = [0], [], np.zeros(col.size, np.int16)
    max_cols = max_entries = 0
    for r0 in range(0, n, rows):
        e0, e1 = rowptr[r0], rowptr[min(r0 + rows, n)]
        cols = np.unique(col[e0:e1])
        lid[e0:e1] = np.searchsorted(cols, col[e0:e1])
        tile_cols.append(cols)
        tile_ptr.append(tile_ptr[-1] + cols.size)
        max_cols, max_entries = max(max_cols, cols.size), max(max_entries, int(e1 - e0))
    return dict(tile_ptr=np.array(tile_ptr, np.int32), tile_cols=np.concatenate(tile_cols).astype(np.int32), lid=lid, rows=rows,
                max_cols=max_cols, max_entries=max_entries)


def _carve_tiles(carve, t, prefix=""):
    v = dict(tile_ptr=carve(prefix + "tile_ptr", I32, t["tile_ptr"].size, "in", t["tile_ptr"]),
             tile_cols=carve(prefix + "tile_cols", I32, t["tile_cols"].size, "in", t["tile_cols"]),
             lid=carve(prefix + "lid", I16, t["lid"].size, "in", t["lid"], floor=0))
    v.update(rows=t["rows"], max_cols=t["max_cols"], max_entries=t["max_entries"])
    return v


def case_graph_from_coo(carve, shape):
    n = shape["n"]
    r, c, val = ring_coo(n, _rng(shape))
    M, cap = len(val), 2 * len(val) + 4 * n
    tr, tc, tv = carve("tri_row", I32, M, "in", r), carve("tri_col", I32, M, "in", c), carve("tri_val", F32, M, "in", val)
    rowptr = carve("rowptr", I32, n + 1, "out")
    col, d2, eid = carve("col", I32, cap, "out", floor=0), carve("d2", F32, cap, "out", floor=0), carve("eid", I32, cap, "out", floor=0)
    q = _lib.lib().mgp_graph_coo_workspace_bytes(n, M)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        nnz = ctypes.c_int64(-7)
        rc = _lib.lib().mgp_graph_from_coo(P(tr), P(tc), P(tv), M, n, P(rowptr), P(col), P(d2), P(eid), ctypes.byref(nnz), P(work),
                                           q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(nnz=np.int64(nnz.value)))
    ext = lambda host: int(host["nnz"])                    # the capacity is an upper bound: the first nnz entries are the CSR
    return Call(run, query=q, extent=dict(col=ext, d2=ext, eid=ext))


def knn_lists(n, k, d, rng):
    """Exact k-NN lists of n random points in float64 (ascending distance, the point itself first), as mgp_knn_search returns them."""
    x = rng.normal(0, 1, (n, d))
    D = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    D[np.arange(n), np.arange(n)] = -1.0
    I = np.argsort(D, 1, kind="stable")[:, :k]
    Dk = np.maximum(np.take_along_axis(D, I, 1), 0.0)
    return Dk.astype(np.float32), I.astype(np.int32)


def case_graph_build(carve, shape):
    n, k = shape["n"], shape["k"]
    Dk, Ik = knn_lists(n, k, 2, _rng(shape))
    D, I = carve("D", F32, n * k, "in", Dk), carve("I", I32, n * k, "in", Ik)
    cap_e = n * (k - 1)
    cap_z = 2 * cap_e + 4 * n
    tr, tc, tv = carve("tri_row", I32, cap_e, "out"), carve("tri_col", I32, cap_e, "out"), carve("tri_val", F32, cap_e, "out")
    rowptr = carve("rowptr", I32, n + 1, "out")
    col, d2, eid = carve("col", I32, cap_z, "out", floor=0), carve("d2", F32, cap_z, "out", floor=0), carve("eid", I32, cap_z, "out", floor=0)
    q = _lib.lib().mgp_graph_workspace_bytes(n, k)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        M, nnz = ctypes.c_int64(-7), ctypes.c_int64(-7)
        rc = _lib.lib().mgp_graph_build(P(D), P(I), n, k, P(tr), P(tc), P(tv), ctypes.byref(M), P(rowptr), P(col), P(d2), P(eid),
                                        ctypes.byref(nnz), P(work), q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(M=np.int64(M.value), nnz=np.int64(nnz.value)))
    em, ez = (lambda host: int(host["M"])), (lambda host: int(host["nnz"]))
    return Call(run, query=q, extent=dict(tri_row=em, tri_col=em, tri_val=em, col=ez, d2=ez, eid=ez))


def case_graph_edges(carve, shape):
    n, k, sym, loop = shape["n"], shape["k"], shape["symmetric"], shape["self_loop"]
    Dk, Ik = knn_lists(n, k, 2, _rng(shape))
    D, I = carve("D", F32, n * k, "in", Dk), carve("I", I32, n * k, "in", Ik)
    cap = n * (k - (0 if loop else 1))
    orow, ocol, oval = carve("out_row", I32, cap, "out"), carve("out_col", I32, cap, "out"), carve("out_val", F32, cap, "out")
    q = _lib.lib().mgp_graph_workspace_bytes(n, k + 1) if sym else 0
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        M = ctypes.c_int64(-7)
        rc = _lib.lib().mgp_graph_edges(P(D), P(I), n, k, sym, loop, P(orow), P(ocol), P(oval), ctypes.byref(M), P(work) if q else None,
                                        q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(M=np.int64(M.value)))
    em = lambda host: int(host["M"])
    return Call(run, query=q, extent=dict(out_row=em, out_col=em, out_val=em))


def case_graph_tiles(carve, shape):
    n, rows, ordered = shape["n"], shape["rows"], shape["ordered"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g, ("rowptr", "col"))
    nnz, ntiles = g["nnz"], -(-n // rows)
    order = carve("row_order", I32, n, "in", rng.permutation(n)) if ordered else None
    tile_rowptr = carve("tile_rowptr", I32, n + 1, "out") if ordered else None
    emap = carve("emap", I32, nnz, "out") if ordered else None
    tile_ptr, tile_cols, lid = carve("tile_ptr", I32, ntiles + 1, "out"), carve("tile_cols", I32, nnz, "out"), carve("lid", I16, nnz, "out")
    q = _lib.lib().mgp_graph_tiles_workspace_bytes(n, nnz)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        total, mc, me = ctypes.c_int64(-7), ctypes.c_int32(-7), ctypes.c_int32(-7)
        rc = _lib.lib().mgp_graph_tiles(n, P(v["rowptr"]), P(v["col"]), nnz, rows, P(order), P(tile_rowptr), P(emap), P(tile_ptr),
                                        P(tile_cols), P(lid), ctypes.byref(total), ctypes.byref(mc), ctypes.byref(me), P(work),
                                        q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(total_cols=np.int64(total.value), max_cols=np.int32(mc.value), max_entries=np.int32(me.value)))
    return Call(run, query=q, extent=dict(tile_cols=lambda host: int(host["total_cols"])))


def case_bfs_order(carve, shape):
    n = shape["n"]
    g = ring_csr(n, _rng(shape))
    v = _carve_csr(carve, g, ("rowptr", "col"))
    order = carve("order", I32, n, "out")
    q = _lib.lib().mgp_graph_bfs_workspace_bytes(n)
    work = carve("work", U8, q, "work", floor=16)
    return _call("mgp_graph_bfs_order", [n, P(v["rowptr"]), P(v["col"]), P(order), P(work), q, _stream()], q, 5)


def case_chain_order(carve, shape):
    n = shape["n"]
    g = ring_csr(n, _rng(shape))
    v = _carve_csr(carve, g, ("rowptr", "col", "d2"))
    order = carve("order", I32, n, "out")
    return _call("mgp_graph_chain_order", [n, P(v["rowptr"]), P(v["col"]), P(v["d2"]), P(order), _stream()])


def case_morton_order(carve, shape):
    n, d = shape["n"], shape["d"]
    x = carve("x", F32, n * d, "in", _rng(shape).normal(0, 1, n * d))
    order = carve("order", I32, n, "out")
    q = _lib.lib().mgp_morton_order_workspace_bytes(n)
    work = carve("work", U8, q, "work", floor=16)
    return _call("mgp_morton_order", [P(x), n, d, P(order), P(work), q, _stream()], q, 5)


def case_laplacian_tangent(carve, shape):
    n = shape["n"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g, ("rowptr", "col", "d2"))
    ins = [carve(k, F32, n, "in", rng.uniform(0.5, 2.0, n)) for k in ("degree_unnorm", "degree", "diag")]
    outs = [carve(k, F32, n, "out") for k in ("d_degree_unnorm", "d_degree", "d_diag", "d_dsqrt", "d_dinvsqrt")]
    d_vals = carve("d_vals", F32, g["nnz"], "out", floor=0)
    args = [n, P(v["rowptr"]), P(v["col"]), P(v["d2"]), 0.8, 0] + [P(t) for t in ins] + [P(t) for t in outs] + [P(d_vals), _stream()]
    return _call("mgp_laplacian_tangent", args)


def case_edge_values(carve, shape):
    n, which = shape["n"], shape["which"]
    rng = _rng(shape)
    r, c, val = ring_coo(n, rng)
    M = len(val)
    tr, tc, tv = carve("tri_row", I32, M, "in", r), carve("tri_col", I32, M, "in", c), carve("tri_val", F32, M, "in", val)
    du, dg = carve("degree_unnorm", F32, n, "in", rng.uniform(0.5, 2, n)), carve("degree", F32, n, "in", rng.uniform(0.5, 2, n))
    out = carve("out", F32, M, "out")
    return _call("mgp_edge_values", [P(tr), P(tc), P(tv), M, P(du), P(dg), 0.8, which, P(out), _stream()])


def case_spmm_backward_sums(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    blocks = _lib.lib().mgp_spmm_backward_blocks(n)
    assert blocks > 0
    ins = [carve(k, F32, n * C, "in", rng.normal(0, 1, n * C)) for k in ("h", "dlx", "xs", "gxs", "X", "g", "lx")]
    partial, gpre, gpost = carve("partial", F32, 2 * blocks, "out"), carve("gpre", F32, n, "out"), carve("gpost", F32, n, "out")
    args = [n, C] + [P(t) for t in ins] + [0.3, 1.1, 0.7, P(partial), P(gpre), P(gpost), _stream()]
    return _call("mgp_spmm_backward_sums", args)


def case_operator_apply_dot(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    op = _operator(g, v)
    X, dotw = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C)), carve("dotw", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "out")
    blocks = _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(op.L), C)
    part = carve("dot_partials", F32, blocks * C, "out")
    q = _lib.lib().mgp_operator_workspace_bytes(ctypes.byref(op), C)
    work = carve("work", U8, q, "work", floor=16)
    call = _call("mgp_operator_apply_dot", [ctypes.byref(op), P(X), C, P(Y), P(dotw), P(part), P(work), q, _stream()], q, 7)
    call.keep = (op,)
    return call


def case_spmm_fused_rows(carve, shape):
    """Rows [r0, r1) of the ring as a local CSR with global column ids; Y is global and only its local rows may change."""
    n, C, r0, r1 = shape["n"], shape["C"], shape["r0"], shape["r1"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    e0, e1 = g["rowptr"][r0], g["rowptr"][r1]
    loc = dict(n=r1 - r0, rowptr=(g["rowptr"][r0:r1 + 1] - e0).astype(np.int32), col=g["col"][e0:e1], vals=g["vals"][e0:e1],
               diag=g["diag"][r0:r1])
    v = _carve_csr(carve, loc)
    csr = _lib.csr_struct(r1 - r0, v["rowptr"], v["col"], v["vals"], v["diag"], ncols=n)
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C))
    pre, post = carve("pre", F32, n, "in", rng.uniform(0.5, 2, n)), carve("post", F32, n, "in", rng.uniform(0.5, 2, n))
    base, dotw = carve("base", F32, n * C, "in", rng.normal(0, 1, n * C)), carve("dotw", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "inout", rng.normal(0, 1, n * C))
    blocks = _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(csr), C)
    part = carve("dot_partials", F32, blocks * C, "out")
    args = [ctypes.byref(csr), r0, P(X), C, P(Y), 0.3, 1.1, P(pre), P(post), P(base), 0.5, 0.9, P(dotw), P(part), _stream()]
    call = _call("mgp_spmm_fused_rows", args)
    call.keep = (csr,)
    return call


def case_spmm_tiled(carve, shape):
    """mgp_spmm_fused on a ring that carries row-tile dictionaries: the family named by shape["choice"] must be the one
    mgp_spmm_kernel_choice reports (rules 1, 2, 4, 5 of the header)."""
    n, C, rows, choice = shape["n"], shape["C"], shape["rows"], shape["choice"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    tv = _carve_tiles(carve, ring_tiles(g, rows))
    csr = _lib.csr_struct(n, v["rowptr"], v["col"], v["vals"], v["diag"], tiles=tv)
    # rules 2-5 refuse operands that are not 16-byte aligned (MGP_ERR_ARG): floor 16 for the blocks, element for the [n] vectors
    fl = 16 if choice in (2, 5, 6) else None
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C), floor=fl)
    pre, post = carve("pre", F32, n, "in", rng.uniform(0.5, 2, n)), carve("post", F32, n, "in", rng.uniform(0.5, 2, n))
    base = carve("base", F32, n * C, "in", rng.normal(0, 1, n * C), floor=fl)
    dotw = carve("dotw", F32, n * C, "in", rng.normal(0, 1, n * C), floor=fl)
    Y = carve("Y", F32, n * C, "out", floor=fl)
    blocks = _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(csr), C)
    assert blocks > 0
    part = carve("dot_partials", F32, blocks * C, "out")
    args = [ctypes.byref(csr), P(X), C, P(Y), 0.3, 1.1, P(pre), P(post), P(base), 0.5, 0.9, P(dotw), P(part), _stream()]
    bar = "bitwise"
    if choice == 0 and C in (4, 8, 12, 16):
        # rule 7: the member follows the alignment of X and Y, and the row16 member (lanes over ENTRIES, partial sums joined by a
        # rotation tree) sums a row in another order than the per-column member.  The bar of the SpMM's float64 tests
        # (test_gpu_past_caps.py): Y within 2e-5 max |ref|; a dot partial within sum |W| 2e-5 max |ref| + 64 x 2^-24 sum |W ref|,
        # taken over all rows -- an upper bound of the same expression over the rows of any one workgroup
        S = np.zeros((n, n))
        np.add.at(S, (np.repeat(np.arange(n), 4), g["col"]), g["vals"].astype(np.float64))
        f64 = lambda t, *sh: t.double().cpu().numpy().reshape(*sh)
        Xs = f64(pre, n, 1) * f64(X, n, C)
        ref = 0.5 * f64(base, n, C) + 0.9 * f64(post, n, 1) * (np.float32(0.3) * Xs + np.float32(1.1) * (g["diag"][:, None] * Xs - S @ Xs))
        scale, W = np.abs(ref).max(), np.abs(f64(dotw, n, C))
        dtol = W.sum(0) * 2e-5 * scale + 64 * 2.0 ** -24 * (W * np.abs(ref)).sum(0)
        bar = ("2e-5 max |ref| for Y and the masked-dot bound for the partials, as test_gpu_past_caps.py",
               {"Y": 2e-5 * scale, "dot_partials": np.tile(dtol, blocks)})
    call = _call("mgp_spmm_fused", args, placement_bar=bar)
    call.keep = (csr,)

    def probe(host):
        got = _lib.lib().mgp_spmm_kernel_choice(ctypes.byref(csr), C, 1, 0)
        assert got == choice, "mgp_spmm_kernel_choice says %d, the family meant is %d" % (got, choice)
    call.probe = probe
    return call


def case_spmm_any(carve, shape):
    return case_spmm_tiled(carve, shape) if "rows" in shape else case_spmm_fused(carve, shape)


# ===================================================================================================================== solvers
def _ring_operator(carve, shape, rng, form=2, tiles=False):
    """An operator on a ring (with 64-row tile dictionaries when `tiles`); returns (g, op, keep)."""
    g = ring_csr(shape["n"], rng)
    v = _carve_csr(carve, g)
    op = _operator(g, v, form=form)
    if tiles:
        tv = _carve_tiles(carve, ring_tiles(g, 64))
        op.L = _lib.csr_struct(g["n"], v["rowptr"], v["col"], v["vals"], v["diag"], tiles=tv)
    return g, op, v


def case_cg_plan(carve, shape):
    """create -> solve (eager) -> solve (captured graph) -> rebind to the same graph at another length scale -> solve -> destroy,
    the workspace carved once at the queried size and watched across the whole sequence."""
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g, op, v = _ring_operator(carve, shape, rng, tiles=shape.get("tiles", False))
    vals2, diag2 = carve("vals2", F32, g["vals"].size, "in", g["vals"] * 0.9, floor=0), carve("diag2", F32, n, "in", g["diag"] * 0.9)
    B = carve("B", F32, n * C, "in", rng.normal(0, 1, n * C))
    X = [carve("X%d" % i, F32, n * C, "out") for i in range(3)]
    q = _lib.lib().mgp_cg_workspace_bytes(ctypes.byref(op), C)
    work = carve("work", U8, q, "work", floor=16)
    params = _lib.CgParamsT(1e-4, 200, 0, 1, 0, 1, 0)
    want = shape.get("probe")

    def run(work_bytes):
        lib, plan, host = _lib.lib(), ctypes.c_void_p(0), {}
        rc = lib.mgp_cg_plan_create(ctypes.byref(op), C, None, ctypes.byref(params), P(work), q if work_bytes is None else work_bytes,
                                    _stream(), ctypes.byref(plan))
        if rc:
            return rc, {}
        try:
            host["folded"], host["complex_shift"] = lib.mgp_cg_plan_is_folded(plan), lib.mgp_cg_plan_is_complex_shift(plan)
            for i in range(3):
                if i == 2:
                    op2 = _operator(g, v)
                    op2.L = op.L
                    op2.L.vals, op2.L.diag, op2.kappa = vals2.data_ptr(), diag2.data_ptr(), 1.3
                    rc = lib.mgp_cg_plan_rebind(plan, ctypes.byref(op2), None)
                    if rc:
                        return rc, {}
                iters, status, resid = ctypes.c_int32(-7), ctypes.c_int32(-7), (ctypes.c_float * C)()
                rc = lib.mgp_cg_plan_solve(plan, P(B), P(X[i]), ctypes.byref(iters), resid, ctypes.byref(status))
                _sync()
                if rc:
                    return rc, {}
                host["iters%d" % i], host["status%d" % i] = np.int32(iters.value), np.int32(status.value)
                host["resid%d" % i] = np.array(list(resid), np.float32)
        finally:
            _sync()
            lib.mgp_cg_plan_destroy(plan)
            _sync()
        return 0, host

    def probe(host):
        assert host["status0"] == 1 and host["status2"] == 1, "the ring solves converge: %s" % host
        for form in ("folded", "complex_shift"):
            assert host[form] == (1 if form == want else 0), "the plan was meant to take %s: %s" % (want or "the plain form", host)
    return Call(run, query=q, probe=probe)


def case_softmax_cg(carve, shape):
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g, op, v = _ring_operator(carve, shape, rng, form=0)
    pi = carve("pi", F32, n * C, "in", _softmax_pi(rng, n, C))
    B = carve("B", F32, n * C, "in", rng.normal(0, 1, n * C))
    X = carve("X", F32, n * C, "out")
    q = _lib.lib().mgp_softmax_cg_workspace_bytes(ctypes.byref(op), C)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        iters, status, resid = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_float(-7.0)
        rc = _lib.lib().mgp_softmax_cg(ctypes.byref(op), P(pi), C, P(B), P(X), 1e-5, 300, 0, ctypes.byref(iters), ctypes.byref(resid),
                                       ctypes.byref(status), P(work), q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(iters=np.int32(iters.value), status=np.int32(status.value), resid=np.float32(resid.value)))
    return Call(run, query=q)


def case_softmax_cg_block(carve, shape):
    n, C, S = shape["n"], shape["C"], shape["S"]
    rng = _rng(shape)
    g, op, v = _ring_operator(carve, shape, rng, form=0)
    pi = carve("pi", F32, n * C, "in", _softmax_pi(rng, n, C))
    B = carve("B", F32, n * S * C, "in", rng.normal(0, 1, n * S * C))
    X = carve("X", F32, n * S * C, "out")
    q = _lib.lib().mgp_softmax_cg_block_workspace_bytes(ctypes.byref(op), C, S)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        iters, resid, status = (ctypes.c_int32 * S)(), (ctypes.c_float * S)(), ctypes.c_int32(-7)
        rc = _lib.lib().mgp_softmax_cg_block(ctypes.byref(op), P(pi), C, S, P(B), P(X), 1e-5, 300, 0, iters, resid, ctypes.byref(status),
                                             P(work), q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(iters=np.array(list(iters), np.int32), resid=np.array(list(resid), np.float32),
                                       status=np.int32(status.value)))
    return Call(run, query=q)


def case_lanczos_tridiag(carve, shape):
    n, steps = shape["n"], shape["steps"]
    rng = _rng(shape)
    g, op, v = _ring_operator(carve, shape, rng)
    q0 = carve("q0", F32, n, "in", rng.normal(0, 1, n))
    Q = carve("Q_out", F32, steps * n, "out")
    q = _lib.lib().mgp_lanczos_tridiag_workspace_bytes(ctypes.byref(op), steps)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        alpha, beta = (ctypes.c_float * steps)(), (ctypes.c_float * steps)()
        rc = _lib.lib().mgp_lanczos_tridiag(ctypes.byref(op), P(q0), steps, alpha, beta, P(Q), P(work),
                                            q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(alpha=np.array(list(alpha), np.float32), beta=np.array(list(beta), np.float32)))
    return Call(run, query=q)


def case_lanczos_tridiag_block(carve, shape):
    n, Pc, steps = shape["n"], shape["P"], shape["steps"]
    rng = _rng(shape)
    g, op, v = _ring_operator(carve, shape, rng)
    Q0 = carve("Q0", F32, n * Pc, "in", rng.normal(0, 1, n * Pc))
    q = _lib.lib().mgp_lanczos_tridiag_block_workspace_bytes(ctypes.byref(op), Pc, steps)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        alpha, beta = (ctypes.c_float * (steps * Pc))(), (ctypes.c_float * (steps * Pc))()
        rc = _lib.lib().mgp_lanczos_tridiag_block(ctypes.byref(op), P(Q0), Pc, steps, alpha, beta, P(work),
                                                  q if work_bytes is None else work_bytes, _stream())
        _sync()
        return rc, ({} if rc else dict(alpha=np.array(list(alpha), np.float32), beta=np.array(list(beta), np.float32)))
    return Call(run, query=q)


def case_blz(carve, shape):
    """mgp_blz_begin -> steps x (read q_j inside the workspace, W = diag(a) q_j, mgp_blz_step) -> mgp_blz_end on one workspace."""
    n, Pc, steps = shape["n"], shape["P"], shape["steps"]
    rng = _rng(shape)
    Q0 = carve("Q0", F32, n * Pc, "in", rng.normal(0, 1, n * Pc))
    a = carve("a", F32, n, "in", rng.uniform(0.5, 3.0, n))
    W = carve("W", F32, n * Pc, "inout", np.zeros(n * Pc))
    q = _lib.lib().mgp_blz_workspace_bytes(n, Pc, steps)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        lib, wb, st = _lib.lib(), q if work_bytes is None else work_bytes, _stream()
        rc = lib.mgp_blz_begin(P(Q0), n, Pc, steps, P(work), wb, st)
        if rc:
            return rc, {}
        for j in range(steps):
            off = int(lib.mgp_blz_q(n, Pc, steps, j, P(work), wb)) - work.data_ptr()
            assert 0 <= off and off + 4 * n * Pc <= q, "mgp_blz_q points outside the workspace"
            qj = work[off:off + 4 * n * Pc].view(F32).view(n, Pc)
            W.view(n, Pc).copy_(qj * a[:, None])
            rc = lib.mgp_blz_step(P(W), n, Pc, steps, j, P(work), wb, st)
            if rc:
                return rc, {}
        alpha, beta = (ctypes.c_float * (steps * Pc))(), (ctypes.c_float * (steps * Pc))()
        rc = lib.mgp_blz_end(n, Pc, steps, alpha, beta, P(work), wb, st)
        _sync()
        return rc, ({} if rc else dict(alpha=np.array(list(alpha), np.float32), beta=np.array(list(beta), np.float32)))
    return Call(run, query=q)


def case_lanczos_smallest(carve, shape):
    """mgp_lanczos_smallest / _ex / _warm (shape["entry"]); the warm start is the exact block of a float64 eigh."""
    n, m, entry = shape["n"], shape["m"], shape["entry"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    csr = _csr_struct(g, v)
    prm = _lib.LanczosParamsT(0, 0, 0, 1e-4, 1337)
    b = min(_lib.lib().mgp_lanczos_block_size(m, ctypes.byref(prm)), n)
    evecs = carve("evecs", F32, n * m, "out")
    bvec = carve("block_evecs", F32, n * b, "out") if entry != "plain" else None
    warm = None
    if entry == "warm":
        A = np.zeros((n, n))
        A[np.arange(n), np.arange(n)] = g["diag"]
        np.subtract.at(A, (np.repeat(np.arange(n), 4), g["col"]), g["vals"])
        lam, U = np.linalg.eigh(A)
        warm = carve("warm_block", F32, n * b, "in", U[:, :b] + 1e-3 * rng.normal(0, 1, (n, b)))
        wev = (ctypes.c_float * b)(*lam[:b])
    q = _lib.lib().mgp_lanczos_workspace_bytes(n, m, ctypes.byref(prm))
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        lib, wb = _lib.lib(), q if work_bytes is None else work_bytes
        evals, resid, info = (ctypes.c_float * m)(), (ctypes.c_float * m)(), (ctypes.c_int32 * 4)()
        bev, bres = (ctypes.c_float * b)(), (ctypes.c_float * b)()
        if entry == "plain":
            rc = lib.mgp_lanczos_smallest(ctypes.byref(csr), m, ctypes.byref(prm), evals, P(evecs), resid, info, P(work), wb, _stream())
        elif entry == "ex":
            rc = lib.mgp_lanczos_smallest_ex(ctypes.byref(csr), m, ctypes.byref(prm), evals, P(evecs), resid, info, bev, P(bvec), bres,
                                             P(work), wb, _stream())
        else:
            rc = lib.mgp_lanczos_smallest_warm(ctypes.byref(csr), m, ctypes.byref(prm), evals, P(evecs), resid, info, bev, P(bvec), bres,
                                               P(warm), wev, P(work), wb, _stream())
        _sync()
        return rc, ({} if rc else dict(evals=np.array(list(evals), np.float32), resid=np.array(list(resid), np.float32),
                                       info=np.array(list(info), np.int32), block_evals=np.array(list(bev), np.float32)))
    return Call(run, query=q)


def case_eigvec_postprocess(carve, shape):
    n, m = shape["n"], shape["m"]
    rng = _rng(shape)
    evecs = carve("evecs", F32, n * m, "inout", rng.normal(0, 1, n * m))
    degree = carve("degree", F32, n, "in", rng.uniform(0.5, 2, n))
    wf = _lib.lib().mgp_eigvec_postprocess_work_floats(m)
    work = carve("colnorm_work", F32, wf, "work")
    return _call("mgp_eigvec_postprocess", [P(evecs), n, m, P(degree), P(work), _stream()])


def case_features_oos(carve, shape):
    n, m, T, k = shape["n"], shape["m"], shape["T"], shape["k"]
    rng = _rng(shape)
    evals = carve("evals", F32, m, "in", np.sort(rng.uniform(0, 2, m)))
    evecs = carve("evecs", F32, n * m, "in", rng.normal(0, 1, n * m))
    du, dg = carve("degree_unnorm", F32, n, "in", rng.uniform(0.5, 2, n)), carve("degree", F32, n, "in", rng.uniform(0.5, 2, n))
    d2 = carve("knn_d2", F32, T * k, "in", np.sort(rng.uniform(0.0, 1.0, (T, k)), 1))
    idx = carve("knn_idx", I32, T * k, "in", rng.integers(0, n, (T, k)))
    Z = carve("Z", F32, T * m, "out")
    args = [P(evals), P(evecs), n, m, 2, 0.9, 0.8, shape["normalization"], P(du), P(dg), P(d2), P(idx), T, k, 1.5, 0.5, P(Z), _stream()]
    return _call("mgp_features_oos", args)


def case_spmm_mt(carve, shape):
    """mgp_spmm_mt_fill builds the dense 16-row tile image of a ring from its 16-row dictionaries, mgp_spmm_fused then runs on it:
    family 3 of mgp_spmm_kernel_choice.  dcol and img are an intermediate product of the sequence: watched, not compared."""
    n, C = shape["n"], shape["C"]
    rng = _rng(shape)
    g = ring_csr(n, rng)
    v = _carve_csr(carve, g)
    t16 = ring_tiles(g, 16)
    tv = _carve_tiles(carve, t16, "t16_")
    D = np.diff(t16["tile_ptr"])
    sp = np.concatenate([[0], np.cumsum((D + 63) // 64 * 16)]).astype(np.int32)      # whole bodies of four blocks per tile
    steps, ntiles = int(sp[-1]), len(D)
    sptr = carve("mt_sptr", I32, sp.size, "in", sp)
    dcol, img = carve("mt_dcol", I32, 4 * steps + 192, "work", floor=16), carve("mt_img", F32, 64 * (steps + 32), "work", floor=16)

    class Mt:
        pass
    mt = Mt()
    mt.sptr, mt.dcol, mt.img, mt.tiles, mt.steps = sptr, dcol, img, ntiles, steps
    csr = _lib.csr_struct(n, v["rowptr"], v["col"], v["vals"], v["diag"], mt=mt)
    X = carve("X", F32, n * C, "in", rng.normal(0, 1, n * C), floor=16)
    pre, post = carve("pre", F32, n, "in", rng.uniform(0.5, 2, n)), carve("post", F32, n, "in", rng.uniform(0.5, 2, n))
    base, dotw = carve("base", F32, n * C, "in", rng.normal(0, 1, n * C), floor=16), carve("dotw", F32, n * C, "in", rng.normal(0, 1, n * C), floor=16)
    Y = carve("Y", F32, n * C, "out", floor=16)
    blocks = _lib.lib().mgp_spmm_dot_blocks_csr(ctypes.byref(csr), C)
    assert blocks > 0
    part = carve("dot_partials", F32, blocks * C, "out")

    def run(work_bytes):
        lib = _lib.lib()
        rc = lib.mgp_spmm_mt_fill(n, P(v["rowptr"]), P(v["vals"]), P(tv["lid"]), P(tv["tile_ptr"]), P(tv["tile_cols"]), P(sptr), steps,
                                  P(dcol), P(img), _stream())
        if rc == 0:
            rc = lib.mgp_spmm_fused(ctypes.byref(csr), P(X), C, P(Y), 0.3, 1.1, P(pre), P(post), P(base), 0.5, 0.9, P(dotw), P(part), _stream())
        _sync()
        return rc, {}

    def probe(host):
        got = _lib.lib().mgp_spmm_kernel_choice(ctypes.byref(csr), C, 1, 0)
        assert got == shape["choice"], "mgp_spmm_kernel_choice says %d, the family meant is %d" % (got, shape["choice"])
    return Call(run, probe=probe)


def case_pcg_plan(carve, shape):
    """The single-rank partitioned CG (null communicator): create -> solve -> solve -> destroy, or, with shape["virtual"], one
    virtual rank driven phase by phase (mgp_pcg_plan_enqueue / _poll) on the shared buffer.  The ring is padded with isolated
    nodes to a multiple of the 64-row tile, as parallel.pad_graph does."""
    n, rec, virtual = shape["n"], shape["recurrence"], shape.get("virtual", False)
    rng = _rng(shape)
    g = ring_csr(n, rng)
    n_pad = -(-n // 64) * 64
    g["rowptr"] = np.concatenate([g["rowptr"], np.full(n_pad - n, g["rowptr"][-1], np.int32)])
    g["diag"] = np.concatenate([g["diag"], np.zeros(n_pad - n, np.float32)])
    g["n"] = n_pad
    v = _carve_csr(carve, g)
    tv = _carve_tiles(carve, ring_tiles(g, 64))
    op = _operator(g, v)
    op.L = _lib.csr_struct(n_pad, v["rowptr"], v["col"], v["vals"], v["diag"], tiles=tv)
    b = np.concatenate([rng.normal(0, 1, n), np.zeros(n_pad - n)])
    B = carve("B", F32, n_pad, "in", b)
    X = [carve("X%d" % i, F32, n_pad, "out") for i in range(1 if virtual else 2)]
    sf = _lib.lib().mgp_pcg_shared_floats(n_pad, n_pad, 1) if virtual else 0
    shared = carve("shared", F32, sf, "work", floor=16) if virtual else None
    q = _lib.lib().mgp_pcg_workspace_bytes(n_pad, n_pad, 1)
    work = carve("work", U8, q, "work", floor=16)
    params = _lib.CgParamsT(1e-5, 400, 0, 1, 8, 1, 0)
    rows = (ctypes.c_int64 * 2)(n_pad, n_pad)

    def run(work_bytes):
        lib, plan, host = _lib.lib(), ctypes.c_void_p(0), {}
        rc = lib.mgp_pcg_plan_create(ctypes.byref(op), rows, 0, n_pad, n, None, 0, 1, P(shared), rec, ctypes.byref(params), P(work),
                                     q if work_bytes is None else work_bytes, _stream(), ctypes.byref(plan))
        if rc:
            return rc, {}
        try:
            iters, status, resid = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_float(-7.0)
            if virtual:
                rc = lib.mgp_pcg_plan_enqueue(plan, 0, 0, P(B))
                it, polled = 0, 1
                while rc == 0 and polled == 1 and it <= 400 + 16:
                    for _ in range(8):
                        rc = rc or lib.mgp_pcg_plan_enqueue(plan, 1, it & 1, None)
                        if rec == 1:
                            rc = rc or lib.mgp_pcg_plan_enqueue(plan, 2, it & 1, None)
                        it += 1
                    _sync()
                    polled = lib.mgp_pcg_plan_poll(plan, ctypes.byref(iters), ctypes.byref(resid), ctypes.byref(status))
                if rc or polled:
                    return rc or polled, {}
                off = int(lib.mgp_pcg_plan_x(plan)) - work.data_ptr()
                assert 0 <= off and off + 4 * n_pad <= q, "mgp_pcg_plan_x points outside the workspace"
                X[0].copy_(work[off:off + 4 * n_pad].view(F32))
                host.update(iters=np.int32(iters.value), status=np.int32(status.value), resid=np.float32(resid.value))
            else:
                for i in range(2):
                    rc = lib.mgp_pcg_plan_solve(plan, P(B), P(X[i]), ctypes.byref(iters), ctypes.byref(resid), ctypes.byref(status))
                    _sync()
                    if rc:
                        return rc, {}
                    host["iters%d" % i], host["status%d" % i], host["resid%d" % i] = (np.int32(iters.value), np.int32(status.value),
                                                                                    np.float32(resid.value))
        finally:
            _sync()
            lib.mgp_pcg_plan_destroy(plan)
            _sync()
        return 0, host

    def probe(host):
        assert all(int(val) == 1 for k, val in host.items() if k.startswith("status")), "the ring solve converges: %s" % host
    return Call(run, query=q, probe=probe)


# ======================================================================================================================== k-NN
def case_knn_search(carve, shape):
    """shape["path"]: direct (d < 32), mfma (>= 1024 queries, d >= 32), lowd (d <= 3, N >= 4096), filter (>= 4096 queries against
    >= 16384 points); stats and the fail-over probe say which one ran.  shape["indexed"]: through mgp_knn_index_build and
    mgp_knn_search_indexed."""
    N, nq, d, k, path = shape["N"], shape["nq"], shape["d"], shape["k"], shape["path"]
    rng = _rng(shape)
    xdb = rng.normal(0, 1, (N, d)).astype(np.float32)
    db = carve("db", F32, N * d, "in", xdb)
    if shape.get("self"):
        qv = db
    else:
        qv = carve("q", F32, nq * d, "in", xdb[rng.integers(0, N, nq)] + 0.1 * rng.normal(0, 1, (nq, d)))
    D, I = carve("D", F32, nq * k, "out"), carve("I", I32, nq * k, "out")
    ib = _lib.lib().mgp_knn_index_bytes(N, d) if shape.get("indexed") else 0
    index = carve("index", U8, ib, "work", floor=16) if ib else None       # opaque to the caller: watched, not compared
    q = _lib.lib().mgp_knn_workspace_bytes(N, nq, d, k)
    work = carve("work", U8, q, "work", floor=16)

    def run(work_bytes):
        lib, wb = _lib.lib(), q if work_bytes is None else work_bytes
        stats = (ctypes.c_int64 * 4)(-7, -7, -7, -7)
        if ib:
            rc = 0 if work_bytes is not None else lib.mgp_knn_index_build(P(db), N, d, P(index), ib, _stream())
            if rc:
                return rc, {}
            rc = lib.mgp_knn_search_indexed(P(db), N, d, P(index), ib, P(qv), nq, k, P(D), P(I), P(work), wb, stats, _stream())
        else:
            rc = lib.mgp_knn_search(P(db), N, d, P(qv), nq, k, P(D), P(I), P(work), wb, stats, _stream())
        _sync()
        return rc, ({} if rc else dict(stats=np.array(list(stats), np.int64), failover=np.int64(lib.mgp_knn_last_filter_failover())))

    def probe(host):
        st, fo = host["stats"], int(host["failover"])
        if path == "lowd":
            assert st[3] == -1, "the low-dimensional path reports K' = -1: %s" % st
        elif path == "filter":
            assert st[3] > 0 and fo >= 0, "the candidate filter did not run: stats %s, fail-over %d" % (st, fo)
        else:
            assert st[3] > 0 and fo == -1, "the slab pipeline did not run: stats %s, fail-over %d" % (st, fo)
    return Call(run, query=q, probe=probe)


# ================================================================================================================ dense blocks
def case_kernel_block(carve, shape):
    n1, n2, m = shape["n1"], shape["n2"], shape["m"]
    rng = _rng(shape)
    Z1, Z2 = carve("Z1", F32, n1 * m, "in", rng.normal(0, 1, n1 * m)), carve("Z2", F32, n2 * m, "in", rng.normal(0, 1, n2 * m))
    K = carve("K", F32, n1 * n2, "out")
    # mgp_kernel_block_set_pipe: the kernel is chosen by shape AND 16-byte alignment and the kernels "agree to fp32 rounding".  Two
    # fp32 sums of m products in different orders each carry at most (m + 1) 2^-24 of the sum of the absolute terms (recursive
    # summation, Higham 2002, eq. 3.5), so they differ by at most twice that
    f64 = lambda t: np.abs(t.double().cpu().numpy())
    tol = 2 * (m + 1) * 2.0 ** -24 * 0.7 * (f64(Z1).reshape(n1, m) @ f64(Z2).reshape(n2, m).T)
    bar = ("2 (m + 1) 2^-24 of the sum of the absolute terms: two fp32 summation orders", {"K": tol})
    return _call("mgp_kernel_block", [P(Z1), n1, P(Z2), n2, m, 0.7, P(K), _stream()], placement_bar=bar)


def case_kernel_diag(carve, shape):
    n, m = shape["n"], shape["m"]
    rng = _rng(shape)
    Z1, Z2 = carve("Z1", F32, n * m, "in", rng.normal(0, 1, n * m)), carve("Z2", F32, n * m, "in", rng.normal(0, 1, n * m))
    out = carve("out", F32, n, "out")
    return _call("mgp_kernel_diag", [P(Z1), P(Z2), n, m, 0.7, P(out), _stream()])


def case_features_insample(carve, shape):
    n, m = shape["n"], shape["m"]
    rng = _rng(shape)
    evals = carve("evals", F32, m, "in", np.sort(rng.uniform(0, 2, m)))
    evecs = carve("evecs", F32, n * m, "in", rng.normal(0, 1, n * m))
    Z = carve("Z", F32, n * m, "out")
    return _call("mgp_features_insample", [P(evals), P(evecs), n, m, 2, 0.9, P(Z), _stream()])


def case_lowrank_apply(carve, shape):
    n, m, C = shape["n"], shape["m"], shape["C"]
    rng = _rng(shape)
    Z, X = carve("Z", F32, n * m, "in", rng.normal(0, 1, n * m)), carve("X", F32, n * C, "in", rng.normal(0, 1, n * C))
    Y = carve("Y", F32, n * C, "out")
    q = _lib.lib().mgp_lowrank_workspace_bytes(m, C)
    work = carve("work", U8, q, "work", floor=16)
    return _call("mgp_lowrank_apply", [P(Z), n, m, P(X), C, 0.6, 0.2, P(Y), P(work), q, _stream()], q, 9)


def case_gram_f64(carve, shape):
    n, b = shape["n"], shape["b"]
    rng = _rng(shape)
    A = carve("A", F32, n * b, "in", rng.normal(0, 1, n * b))
    G = carve("G", F64, b * b, "out")
    q = _lib.lib().mgp_gram_workspace_bytes(n, b)
    work = carve("work", U8, q, "work", floor=16)
    return _call("mgp_gram_f64", [P(A), n, b, P(G), P(work), q, _stream()], q, 5)


def case_lowrank_residual(carve, shape):
    n, m, C = shape["n"], shape["m"], shape["C"]
    rng = _rng(shape)
    Z, T = carve("Z", F32, n * m, "in", rng.normal(0, 1, n * m)), carve("T", F64, m * C, "in", rng.normal(0, 1, m * C))
    V = carve("V", F32, n * C, "in", rng.normal(0, 1, n * C))
    out = carve("out", F32, n * C, "out")
    return _call("mgp_lowrank_residual", [P(Z), n, m, P(T), P(V), C, 0.8, P(out), _stream()])


def case_spectral_site(carve, shape):
    """Inputs as tests/test_gpu_spectral_laplace.py builds them (_spectral_laplace_ref.problem)."""
    import _spectral_laplace_ref as sref
    n, m, fam = shape["n"], shape["m"], shape["family"]
    rng = _rng(shape)
    Z64 = sref.f32(rng.standard_normal((n, m)) / np.sqrt(m))
    w64 = 1.5 * rng.standard_normal(m)
    obs = rng.random(n) < 0.5
    obs[0] = True
    d, _ = sref.problem(sref.FAMILIES[fam], 0.7 * (Z64 @ w64), obs, 17 + n + m, mean=0.25)
    Z, w = carve("Z", F32, n * m, "in", Z64), carve("w", F64, m, "in", w64)
    a = carve("a", F32, n, "in", d["a"])
    b = carve("b", F32, n, "in", np.zeros(n) if d["b"] is None else d["b"])
    obsv = carve("obs", U8, n, "in", obs.astype(np.uint8))
    f, grad = carve("f", F64, n, "out"), carve("grad", F64, m, "out")
    hess, sums = carve("hess", F64, m * m, "out"), carve("sums", F64, 2, "out")
    q = _lib.lib().mgp_spectral_site_workspace_bytes(n, m, 1)
    work = carve("work", U8, q, "work", floor=8)
    args = [P(Z), n, m, P(w), fam, P(a), P(b), P(obsv), 0.25, d["r"] or 1.0, P(f), P(grad), P(hess), P(sums), P(work), q, _stream()]
    # 16-byte loads where m % 4 == 0 and Z is 16-byte aligned, scalar ones otherwise (header): "A Z view one float off 16-byte
    # alignment gives the same numbers within the bar" of test_gpu_spectral_laplace.py, 1e-12 of the sum of the absolute terms
    scale = sref.site_outputs(Z64, w64, d)[4]
    tol = {k: 1e-12 * scale[k] for k in ("f", "grad", "hess")}
    tol["sums"] = 1e-12 * np.array([scale["lp"], scale["f"].max()])
    return _call("mgp_spectral_site", args, q, 15,
                 placement_bar=("1e-12 of the sum of the absolute terms, as test_gpu_spectral_laplace.py", tol))


# ==================================================================================================================== families
@contextlib.contextmanager
def knob(setter, value, restore):
    """Sets a lab switch for the run and puts `restore` (its documented default) back in a finally."""
    fn = getattr(_lib.lib(), setter)
    fn(value)
    try:
        yield
    finally:
        fn(restore)


def no_knob():
    return contextlib.nullcontext()


def knobs(*triples):
    """Several switches at once: (setter, value, default) each; all restored in a finally."""
    @contextlib.contextmanager
    def ctx():
        with contextlib.ExitStack() as stack:
            for setter, value, restore in triples:
                stack.enter_context(knob(setter, value, restore))
            yield
    return ctx


class Case:
    """fn: the case function; shapes: {id: shape dict}; families: {id: (context factory, note)} -- the case runs once per family and
    shape; floor / extent / bar: the row of docs/memory_contract.md."""

    def __init__(self, fn, shapes, families=None, floor="element; doubles 8 B off 16", extent="whole arrays", bar="bitwise",
                 reached="one kernel family"):
        self.fn, self.shapes = fn, shapes
        self.families = families or {"default": no_knob}
        self.floor, self.extent, self.bar, self.reached = floor, extent, bar, reached

    def shapes_of(self, family):
        """shapes is {id: shape}, or {family: {id: shape}} where every family needs a shape of its own to be reached."""
        return self.shapes[family] if set(self.shapes) == set(self.families) else self.shapes


def _n(*extra):
    """n = 1 and n = 257 (1 mod 4, just past one 256-lane workgroup), crossed with the extra shape dicts."""
    out = {}
    for n in (1, 257):
        for e in (extra or ({},)):
            d = dict(n=n, **e)
            out["-".join("%s%s" % (k, v) for k, v in d.items() if not isinstance(v, (tuple, list)))] = d
    return out


def _rings(*extra):
    """Rings of 3 nodes (the smallest) and 257."""
    out = {}
    for n in (3, 257):
        for e in (extra or ({},)):
            d = dict(n=n, **e)
            out["-".join("%s%s" % (k, v) for k, v in d.items())] = d
    return out


SITE_FLOOR = "float arrays one element off 16 B (scalar path), obs 1 B, doubles 8 B off 16, work 8 B"
CASES = {
    "mgp_bernoulli_site": Case(_newton("mgp_bernoulli_site", "mgp_bernoulli_site_workspace_bytes", ["y01"], (0.1, 0)), _n(),
                               floor=SITE_FLOOR, extent="w, rhs [n]; sums [4]"),
    "mgp_count_site": Case(_newton("mgp_count_site", "mgp_count_site_workspace_bytes", ["counts", "trials"], None),
                           {**{k + "-poisson": dict(v, scalars=(0.1, 0.2, 0)) for k, v in _n().items()},
                            **{k + "-binomial": dict(v, scalars=(0.1, 0.2, 1)) for k, v in _n().items()}},
                           floor=SITE_FLOOR, extent="w, rhs [n]; sums [4]"),
    "mgp_nb_site": Case(_newton("mgp_nb_site", "mgp_nb_site_workspace_bytes", ["counts", "logexp"], (0.1, 0.2, 3.5)), _n(),
                        floor=SITE_FLOOR, extent="w, rhs [n]; sums [4]"),
    "mgp_ordinal_site": Case(_newton("mgp_ordinal_site", "mgp_ordinal_site_workspace_bytes", ["lo", "hi"], (0.1,)), _n(),
                             floor=SITE_FLOOR, extent="w, rhs [n]; sums [4]"),
    "mgp_laplace_evidence_site": Case(
        _evidence("mgp_laplace_evidence_site", "mgp_laplace_evidence_site_workspace_bytes", ["counts", "trials"], None),
        {"%s-family%d" % (k, fam): dict(v, scalars=(0.2, fam, 1e-6)) for k, v in _n().items() for fam in (0, 1, 2)},
        floor=SITE_FLOOR, extent="root_h, corr [n]; sums [4]"),
    "mgp_nb_evidence_site": Case(_evidence("mgp_nb_evidence_site", "mgp_nb_evidence_site_workspace_bytes", ["counts", "logexp"],
                                           (0.2, 3.5, 1e-6)), _n(), floor=SITE_FLOOR, extent="root_h, corr [n]; sums [4]"),
    "mgp_ordinal_evidence_site": Case(_evidence("mgp_ordinal_evidence_site", "mgp_ordinal_evidence_site_workspace_bytes", ["lo", "hi"],
                                                (1e-6,)), _n(), floor=SITE_FLOOR, extent="root_h, corr [n]; sums [4]"),
    "mgp_nb_dispersion_sums": Case(case_nb_dispersion_sums, _n(), floor=SITE_FLOOR, extent="out [3] (the array has three entries)"),
    "mgp_ordinal_cut_sums": Case(case_ordinal_cut_sums, _n(dict(K=2), dict(K=5), dict(K=64)), floor="element; work 8 B",
                                 extent="out [3, K - 1]"),
    "mgp_softmax_site": Case(case_softmax_site, _n(dict(C=2), dict(C=3), dict(C=37), dict(C=64)), floor="element; work 8 B",
                             extent="pi, rhs [n, C]; sums [4]"),
    "mgp_softmax_hessian_add": Case(case_softmax_hessian_add, _n(dict(C=2), dict(C=3), dict(C=37), dict(C=64)),
                                    extent="Y [n, C] in/out"),
    "mgp_softmax_hessian_add_block": Case(case_softmax_hessian_add_block, _n(dict(C=3, S=5), dict(C=37, S=6), dict(C=2, S=1)),
                                          floor="element; work 16 B", extent="Y [n, S, C] in/out; sums [S, 2]"),
    "mgp_softmax_root_apply": Case(case_softmax_root_apply,
                                   _n(dict(C=3, S=5, layout="ncs", transpose=0), dict(C=3, S=5, layout="nsc", transpose=1),
                                      dict(C=37, S=6, layout="ncs", transpose=1), dict(C=64, S=1, layout="nsc", transpose=0)),
                                   extent="out [n, C, S]"),
    "mgp_softmax_curvature": Case(case_softmax_curvature, _n(dict(C=3, S=5), dict(C=37, S=6), dict(C=2, S=1)),
                                  extent="acc, acc2 [n, C] in/out"),
    "mgp_scale_rows": Case(case_scale_rows, _n(dict(P=1, with_x=0), dict(P=7, with_x=1), dict(P=12, with_x=1), dict(P=256, with_x=0)),
                           extent="out [n, P]", reached="float4 form at P % 4 == 0 and aligned placement, scalar form otherwise"),
    "mgp_row_moments": Case(case_row_moments, _n(dict(C=1), dict(C=7), dict(C=12), dict(C=256)), extent="acc [n, 2] in/out",
                            bar="fills bitwise; placement 1e-12 of the sum of the absolute terms (float4 / scalar loads)",
                            reached="float4 loads at C % 4 == 0 and aligned placement, scalar loads otherwise"),
    "mgp_bernoulli_predict": Case(case_bernoulli_predict, _n(dict(points=9), dict(points=65)), extent="prob [n]"),
    "mgp_ordinal_predict": Case(case_ordinal_predict, _n(dict(K=2, points=9, log_out=0), dict(K=5, points=65, log_out=1),
                                                         dict(K=64, points=33, log_out=0)), extent="out [n, K]"),
    "mgp_count_predict_pmf": Case(case_count_predict_pmf, _n(dict(family=0, K=1, k0=0, points=17), dict(family=1, K=70, k0=2, points=33)),
                                  extent="out [n, K]"),
    "mgp_count_predict_logpmf": Case(case_count_predict_logpmf, _n(dict(family=0, points=17), dict(family=1, points=33)),
                                     extent="out [n]"),
    "mgp_nb_predict_pmf": Case(case_nb_predict_pmf, _n(dict(K=1, k0=0, points=17), dict(K=70, k0=2, points=33)), extent="out [n, K]"),
    "mgp_nb_predict_logpmf": Case(case_nb_predict_logpmf, _n(dict(points=17), dict(points=33)), extent="out [n]"),
    "mgp_permute_rows": Case(case_permute_rows, _n(dict(C=1), dict(C=7), dict(C=12)), extent="dst [n, C]"),
    "mgp_laplacian_build": Case(case_laplacian_build, _rings(), floor="element; col, d2, vals 16 B (quad loads)",
                                extent="five [n] vectors; vals [nnz]"),
    "mgp_spmm_fused": Case(
        case_spmm_any,
        {"gather": _rings(dict(C=1), dict(C=5), dict(C=20)),
         "gather-v4-always": _rings(dict(C=20)), "gather-v4-never": _rings(dict(C=20)),
         "tile-c1": _rings(dict(C=1, rows=32, choice=1), dict(C=1, rows=64, choice=1), dict(C=1, rows=128, choice=1)),
         "tile-c1-loop": _rings(dict(C=1, rows=64, choice=1)),
         "tile-off": _rings(dict(C=1, rows=64, choice=0)),
         "tile-small": _rings(dict(C=4, rows=64, choice=2), dict(C=12, rows=64, choice=2), dict(C=16, rows=64, choice=2)),
         "tile-small-off": _rings(dict(C=12, rows=64, choice=0)),
         # (the dictionary kernel wants slices of >= 32 slots: a tile with at least 17 distinct columns, so no ring of 3)
         "dict": {"n131-C68": dict(n=131, C=68, rows=64, choice=5), "n257-C68": dict(n=257, C=68, rows=64, choice=5),
                  "n257-C256": dict(n=257, C=256, rows=64, choice=5)},
         "tile-wide": _rings(dict(C=20, rows=64, choice=6))},
        families={"gather": no_knob, "gather-v4-always": lambda: knob("mgp_spmm_set_v4_mode", 2, 1),
                  "gather-v4-never": lambda: knob("mgp_spmm_set_v4_mode", 0, 1),
                  "tile-c1": no_knob, "tile-c1-loop": lambda: knob("mgp_spmm_set_tile_loop_mode", 1, 0),
                  "tile-off": lambda: knob("mgp_spmm_set_tile_mode", 0, 1), "tile-small": no_knob,
                  "tile-small-off": lambda: knob("mgp_spmm_set_tile_small_mode", 0, 1),
                  "dict": lambda: knob("mgp_spmm_set_dict_mode", 2, 1),
                  "tile-wide": knobs(("mgp_spmm_set_dict_mode", 0, 1), ("mgp_spmm_set_tile_wide_mode", 2, 1))},
        floor="element ([n] vectors, blocks of rules 1, 6, 7); 16 B for col, vals, lid and for the blocks of rules 2-5 (MGP_ERR_ARG below)",
        extent="Y [n, C]; dot_partials [mgp_spmm_dot_blocks_csr, C]",
        bar="bitwise; placement at rule 7 with C in {4, 8, 12, 16}: Y 2e-5 max |ref|, partials the masked-dot bound (row16 member)",
        reached="mgp_spmm_kernel_choice: 0 (row groups, gather members), 1 (C = 1 tiles of 32 / 64 / 128 rows, tile-loop form), 2 (small-C "
                "tiles), 5 (dictionary, dict mode 2), 6 (chunked dictionary, wide mode 2)"),
    "mgp_operator_apply": Case(case_operator_apply, _rings(dict(C=1), dict(C=5), dict(C=1, form=1)), floor="element; work 16 B",
                               extent="Y [n, C]"),
    "mgp_operator_jacobi": Case(case_operator_jacobi, _rings(), extent="minv [n]"),
    "mgp_operator_apply_double": Case(case_operator_apply_double, _rings(dict(C=1), dict(C=3)), floor="doubles 8 B off 16; work 8 B",
                                      extent="Y [n, C]"),
    "mgp_operator_diag_exact": Case(case_operator_diag_exact, _rings(dict(nu=1), dict(nu=2), dict(nu=3)), extent="diag_out [n]"),
    "mgp_gmrf_noise": Case(case_gmrf_noise, _rings(dict(S=1), dict(S=7)), extent="Y [n, S]"),
    "mgp_laplacian_matmul": Case(case_laplacian_matmul, _rings(dict(C=1, mode=0), dict(C=5, mode=1), dict(C=5, mode=2)),
                                 extent="Y [n, C]"),
    "mgp_cg_solve": Case(case_cg_solve, _rings(dict(C=1), dict(C=5)), floor="element; work 16 B", extent="X [n, C]; iters, resid [C]"),
    "mgp_graph_from_coo": Case(case_graph_from_coo, _rings(), floor="element; col, d2, eid 16 B; work 16 B",
                               extent="rowptr [n + 1]; col, d2, eid: the first nnz of a capacity 2 M + 4 n"),
    "mgp_graph_build": Case(case_graph_build, {"n3-k2": dict(n=3, k=2), "n257-k5": dict(n=257, k=5), "n257-k11": dict(n=257, k=11)},
                            floor="element; col, d2, eid 16 B; work 16 B",
                            extent="tri_* : the first M of n (k - 1); rowptr [n + 1]; col, d2, eid: the first nnz of 2 n (k - 1) + 4 n"),
    "mgp_graph_edges": Case(case_graph_edges,
                            {"n%d-k%d-sym%d-loop%d" % (n, k, sy, lp): dict(n=n, k=k, symmetric=sy, self_loop=lp)
                             for n, k in ((3, 2), (257, 5)) for sy in (0, 1) for lp in (0, 1)},
                            floor="element; work 16 B", extent="out_* : the first M of n (k - first)"),
    "mgp_graph_tiles": Case(case_graph_tiles,
                            {"n%d-rows%d-ordered%d" % (n, r, o): dict(n=n, rows=r, ordered=o) for n in (3, 257) for r, o in ((64, 0), (16, 0), (64, 1))},
                            floor="element; col 16 B; work 16 B",
                            extent="tile_ptr [ntiles + 1]; tile_cols: the first total_cols of nnz; lid [nnz]; tile_rowptr [n + 1], emap [nnz]"),
    "mgp_graph_bfs_order": Case(case_bfs_order, _rings(), floor="element; col 16 B; work 16 B", extent="order [n]"),
    "mgp_graph_chain_order": Case(case_chain_order, _rings(), floor="element; col, d2 16 B", extent="order [n]"),
    "mgp_morton_order": Case(case_morton_order, _n(dict(d=1), dict(d=2), dict(d=3)), floor="element; work 16 B", extent="order [n]"),
    "mgp_laplacian_tangent": Case(case_laplacian_tangent, _rings(), floor="element; col, d2, d_vals 16 B",
                                  extent="five [n] vectors; d_vals [nnz]"),
    "mgp_edge_values": Case(case_edge_values, _rings(dict(which=0), dict(which=1), dict(which=2)), extent="out [M]"),
    "mgp_spmm_backward_sums": Case(case_spmm_backward_sums, _n(dict(C=1), dict(C=5), dict(C=12)),
                                   extent="partial [mgp_spmm_backward_blocks, 2]; gpre, gpost [n]"),
    "mgp_operator_apply_dot": Case(case_operator_apply_dot, _rings(dict(C=1), dict(C=5)), floor="element; work 16 B",
                                   extent="Y [n, C]; dot_partials [mgp_spmm_dot_blocks_csr, C]"),
    "mgp_spmm_fused_rows": Case(case_spmm_fused_rows,
                                {"n257-C1-rows64-193": dict(n=257, C=1, r0=64, r1=193), "n257-C5-rows0-7": dict(n=257, C=5, r0=0, r1=7),
                                 "n257-C5-rows250-257": dict(n=257, C=5, r0=250, r1=257)},
                                floor="element; col, vals 16 B", extent="Y [n, C] in/out: only rows [r0, r1) may change; dot_partials"),
    "mgp_spmm_mt_fill": Case(case_spmm_mt,
                             {"matrix-core": {"n3-C48": dict(n=3, C=48, choice=3), "n257-C68": dict(n=257, C=68, choice=3),
                                              "n257-C256": dict(n=257, C=256, choice=3)},
                              "mt-off": {"n257-C68": dict(n=257, C=68, choice=0)}},
                             families={"matrix-core": no_knob, "mt-off": lambda: knob("mgp_spmm_set_mt_mode", 0, 1)},
                             floor="element; col, vals, lid, dcol, img and the blocks 16 B",
                             extent="Y [n, C]; dot_partials; dcol [4 steps + 192] and img [64 (steps + 32)] watched, not compared",
                             reached="mgp_spmm_kernel_choice == 3 (matrix-core tiles); 0 with mt mode 0"),
    "mgp_pcg_plan_create": Case(case_pcg_plan,
                                {"n%d-rec%d%s" % (n, r, "-virtual" if vr else ""): dict(n=n, recurrence=r, virtual=vr)
                                 for n in (257, 320) for r in (0, 1) for vr in (False, True)},
                                floor="element; col, vals, lid 16 B; shared, work 16 B",
                                extent="X_loc [n_loc] of both solves; the virtual rank's solution inside the workspace; iters, resid, status"),
    "mgp_cg_plan_create": Case(
        case_cg_plan,
        {"gather": _rings(dict(C=1, probe="complex_shift"), dict(C=5)),
         "complex-shift": _rings(dict(C=1, tiles=True, probe="complex_shift")),
         "folded": _rings(dict(C=1, tiles=True, probe="folded")),
         "classic-c1": _rings(dict(C=1, tiles=True)),
         "update-elements": _rings(dict(C=12)), "reduce-every": _rings(dict(C=20)), "wide": _rings(dict(C=20))},
        families={"gather": no_knob, "complex-shift": no_knob,
                  "folded": knobs(("mgp_cg_set_complex_shift", 0, 1), ("mgp_cg_set_fold_update", 2, 1)),
                  "classic-c1": knobs(("mgp_cg_set_complex_shift", 0, 1), ("mgp_cg_set_fold_update", 0, 1), ("mgp_cg_set_init_free", 0, 1),
                                      ("mgp_cg_set_decide_in_update", 0, 1)),
                  "update-elements": lambda: knob("mgp_cg_set_update_quads", 0, 1),
                  "reduce-every": lambda: knob("mgp_cg_set_reduce_once", 0, 1), "wide": no_knob},
        floor="element; col, vals, lid 16 B; work 16 B", extent="X [n, C] of each of the three solves; iters, resid, status",
        reached="mgp_cg_plan_is_complex_shift, mgp_cg_plan_is_folded; the other switches have no probe"),
    "mgp_softmax_cg": Case(case_softmax_cg, _rings(dict(C=2), dict(C=3), dict(C=37)), floor="element; work 16 B",
                           extent="X [n, C]; iters, resid, status"),
    "mgp_softmax_cg_block": Case(case_softmax_cg_block, _rings(dict(C=3, S=5), dict(C=37, S=6), dict(C=2, S=1)), floor="element; work 16 B",
                                 extent="X [n, S, C]; iters [S], resid [S], status"),
    "mgp_lanczos_tridiag": Case(case_lanczos_tridiag, {"n3-steps2": dict(n=3, steps=2), "n257-steps7": dict(n=257, steps=7)},
                                floor="element; work 16 B", extent="Q_out [steps, n]; alpha, beta [steps]"),
    "mgp_lanczos_tridiag_block": Case(case_lanczos_tridiag_block,
                                      {"n3-P1-steps2": dict(n=3, P=1, steps=2), "n257-P5-steps7": dict(n=257, P=5, steps=7),
                                       "n257-P16-steps6": dict(n=257, P=16, steps=6)},
                                      floor="element; work 16 B", extent="alpha, beta [steps, P]"),
    "mgp_blz_begin": Case(case_blz, {"n3-P1-steps2": dict(n=3, P=1, steps=2), "n257-P5-steps7": dict(n=257, P=5, steps=7),
                                     "n257-P16-steps6": dict(n=257, P=16, steps=6)},
                          floor="element; work 16 B", extent="W [n, P] in/out; alpha, beta [steps, P]"),
    "mgp_lanczos_smallest": Case(case_lanczos_smallest, {"n3-m1": dict(n=3, m=1, entry="plain"), "n257-m3": dict(n=257, m=3, entry="plain")},
                                 floor="element; col, vals 16 B; work 16 B", extent="evecs [n, m]; evals, resid [m], info [4]"),
    "mgp_lanczos_smallest_ex": Case(case_lanczos_smallest, {"n3-m1": dict(n=3, m=1, entry="ex"), "n257-m3": dict(n=257, m=3, entry="ex")},
                                    floor="element; col, vals 16 B; work 16 B", extent="evecs [n, m]; block_evecs [n, b]; host arrays"),
    "mgp_lanczos_smallest_warm": Case(case_lanczos_smallest, {"n3-m1": dict(n=3, m=1, entry="warm"), "n257-m3": dict(n=257, m=3, entry="warm")},
                                      floor="element; col, vals 16 B; work 16 B", extent="evecs [n, m]; block_evecs [n, b]; host arrays"),
    "mgp_eigvec_postprocess": Case(case_eigvec_postprocess, {"n1-m1": dict(n=1, m=1), "n257-m7": dict(n=257, m=7), "n257-m20": dict(n=257, m=20)},
                                   extent="evecs [n, m] in/out; colnorm_work is scratch"),
    "mgp_features_oos": Case(case_features_oos,
                             {"n3-m1-T1-k1": dict(n=3, m=1, T=1, k=1, normalization=0), "n257-m7-T33-k5": dict(n=257, m=7, T=33, k=5, normalization=1),
                              "n257-m20-T257-k11": dict(n=257, m=20, T=257, k=11, normalization=0)}, extent="Z [T, m]"),
    "mgp_knn_search": Case(
        case_knn_search,
        {"direct": {"N1": dict(N=1, nq=1, d=1, k=1, path="direct"), "N300-q77-d5": dict(N=300, nq=77, d=5, k=7, path="direct"),
                    "self-N257-d7": dict(N=257, nq=257, d=7, k=5, path="direct", self=True),
                    "N300-q77-d33": dict(N=300, nq=77, d=33, k=7, path="direct")},
         "mfma": {"self-1100x33": dict(N=1100, nq=1100, d=33, k=7, path="mfma", self=True),
                  "N1100-q1030-d33": dict(N=1100, nq=1030, d=33, k=7, path="mfma")},
         "mfma-full-tiles": {"self-1100x33": dict(N=1100, nq=1100, d=33, k=7, path="mfma", self=True)},
         "mfma-off": {"self-1100x33": dict(N=1100, nq=1100, d=33, k=7, path="mfma", self=True)},
         "lowd": {"self-4100x3": dict(N=4100, nq=4100, d=3, k=5, path="lowd", self=True),
                  "N4100-q33-d2": dict(N=4100, nq=33, d=2, k=5, path="lowd")},
         "filter": {"N16384-q4096-d32": dict(N=16384, nq=4096, d=32, k=7, path="filter")},
         "filter-forced": {"self-1100x33": dict(N=1100, nq=1100, d=33, k=7, path="filter", self=True)}},
        families={"direct": no_knob, "mfma": no_knob, "mfma-full-tiles": lambda: knob("mgp_knn_set_symmetric", 0, 1),
                  "mfma-off": lambda: knob("mgp_knn_set_mfma", 0, 1), "lowd": no_knob, "filter": no_knob,
                  "filter-forced": lambda: knob("mgp_knn_set_filter", 2, 1)},
        floor="element; work 16 B", extent="D, I [n, k]; stats [4]",
        reached="stats[3] (K' > 0: slab or filter, -1: low dimension) and mgp_knn_last_filter_failover (-1: slab, >= 0: filter); no probe "
                "tells the matrix-core keys from the direct tiles"),
    "mgp_knn_index_build": Case(case_knn_search, {"N1100-q77-d33": dict(N=1100, nq=77, d=33, k=7, path="mfma", indexed=True),
                                                  "N1100-q1-d33": dict(N=1100, nq=1, d=33, k=7, path="mfma", indexed=True)},
                                floor="element; index, work 16 B", extent="D, I [n, k]; the index is opaque (watched, not compared)"),
    "mgp_kernel_block": Case(case_kernel_block,
                             {"1x1x1": dict(n1=1, n2=1, m=1), "257x33x7": dict(n1=257, n2=33, m=7), "129x132x20": dict(n1=129, n2=132, m=20),
                              "260x36x16": dict(n1=260, n2=36, m=16)},
                             families={"pipe%d" % p: (lambda p=p: knob("mgp_kernel_block_set_pipe", p, 0)) for p in (0, 1, 2, 4)},
                             extent="K [n1, n2]", bar="fills bitwise; placement 2 (m + 1) 2^-24 of the sum of the absolute terms",
                             reached="pipe 0, 1, 2, 4; no probe exists for the kernel taken"),
    "mgp_kernel_diag": Case(case_kernel_diag, {"n1-m1": dict(n=1, m=1), "n257-m7": dict(n=257, m=7), "n257-m20": dict(n=257, m=20)},
                            extent="out [n]"),
    "mgp_features_insample": Case(case_features_insample, {"n1-m1": dict(n=1, m=1), "n257-m7": dict(n=257, m=7),
                                                           "n257-m20": dict(n=257, m=20)}, extent="Z [n, m]"),
    "mgp_lowrank_apply": Case(case_lowrank_apply, {"n1": dict(n=1, m=1, C=1), "n257-m7-C3": dict(n=257, m=7, C=3),
                                                   "n257-m20-C1": dict(n=257, m=20, C=1)}, floor="element; work 16 B", extent="Y [n, C]"),
    "mgp_gram_f64": Case(case_gram_f64, {"n1-b1": dict(n=1, b=1), "n257-b7": dict(n=257, b=7), "n1030-b21": dict(n=1030, b=21)},
                         families={"mfma": no_knob, "vector": lambda: knob("mgp_gram_set_mfma", 0, 1)}, floor="element; work 16 B",
                         extent="G [b, b]", reached="fp64 matrix cores and fp64 vector FMAs (mgp_gram_set_mfma)"),
    "mgp_lowrank_residual": Case(case_lowrank_residual, {"n1": dict(n=1, m=1, C=1), "n257-m7-C3": dict(n=257, m=7, C=3)},
                                 extent="out [n, C]"),
    "mgp_spectral_site": Case(case_spectral_site,
                              {"n%d-m%d-family%d" % (n, m, fam): dict(n=n, m=m, family=fam)
                               for n, m, fam in ((1, 1, 0), (257, 7, 1), (257, 20, 2), (257, 33, 3), (33, 5, 4))},
                              floor="Z one element off 16 B (scalar loads); doubles 8 B off 16; work 8 B",
                              extent="f [n]; grad [m]; hess [m, m]; sums [2]",
                              bar="fills bitwise; placement 1e-12 of the sum of the absolute terms (16-byte / scalar loads of Z)"),
}

# ===================================================================================================================== exempt
EXEMPT_CATEGORIES = {
    "size query": r".*_workspace_bytes$|.*_index_bytes$|.*_work_floats$|^mgp_pcg_shared_floats$|^mgp_spmm_dot_blocks(_csr)?$|"
                  r"^mgp_spmm_backward_blocks$|^mgp_dist_unique_id_bytes$",
    "knob or probe": r".*_set_.*|^mgp_spmm_kernel_choice$|^mgp_lanczos_block_size$|.*_plan_is_.*|.*_last_.*|^mgp_spmm_timing_(begin|end)$|"
                     r"^mgp_version$|^mgp_device_info$",
    "plan lifecycle": r".*_plan_(destroy|poison|poisoned|poll)$",
    "pointer getter": r"^mgp_blz_q$|.*_plan_x(64)?$",
    "host-only routine": r"^mgp_host_symeig$",
    "benchmark loop": r"^mgp_spmm_repeat$",
    "takes a communicator": r"^mgp_dist_.*|^mgp_cg_plan_create_dist$|^mgp_operator_apply_part$",
}


def _category(name):
    for cat, pat in EXEMPT_CATEGORIES.items():
        if re.match(pat, name):
            return cat
    return None


EXEMPT = {name: _category(name) for name in _lib.SIGNATURES if _category(name) is not None}

# Entry points exercised inside another entry point's case: the plan and block-Lanczos sequences are one case each.
COVERED_BY = {
    "mgp_cg_plan_solve": "mgp_cg_plan_create", "mgp_cg_plan_rebind": "mgp_cg_plan_create",
    "mgp_blz_step": "mgp_blz_begin", "mgp_blz_end": "mgp_blz_begin",
    "mgp_knn_search_indexed": "mgp_knn_index_build",
    "mgp_pcg_plan_solve": "mgp_pcg_plan_create", "mgp_pcg_plan_enqueue": "mgp_pcg_plan_create",
}

# Entry points that launch device work on caller memory and have no case yet: none.  A new entry point lands here, with its
# reason, only until its case exists (docs/memory_contract.md lists it).
PENDING = {}


def params():
    """(entry point, family id, shape id) of every run, in registry order."""
    return [(name, fam, sid) for name, c in CASES.items() for fam in c.families for sid in c.shapes_of(fam)]
