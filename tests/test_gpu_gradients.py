"""The hyper-parameter gradient path on the GPU against float64 (oracle/grad_ref.py), at the launch geometry that training at
size runs on.

  a  mgp_laplacian_tangent (lap_tangent_pass) entry by entry, on the golden graphs, a star-plus-ring graph with one long row, and a
     150k-node swiss roll past both grid caps (4096 x 16 rows of the tangent passes, 512 x 256 rows of the backward sums); on the
     same graphs the VALUES it differentiates -- the six arrays of mgp_laplacian_build and the per-edge W, A, S of
     mgp_edge_values -- entry by entry in the same form and at the same bar;
  b  one differentiable fused SpMM (autograd.fused_spmm) and all nine of its gradients, at C = 1 ... 300, natural and locality
     row order, with the fused backward reductions on and off;
  c  mgp_spmm_backward_sums called directly against float64 numpy, every legal null pattern, every illegal one refused;
  d  <W, Q3 V> through the operators (Noise(Scale(Precision(L)))) and its gradients, on the golden graphs.

Every case asserts that the path it targets ran (row counts past the caps, a locality order, the kernel family).  The measured
worst ratios (error / bound) are recorded in each docstring and in docs/kernels/gradients.md.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from oracle.grad_ref import (NAMES, bilinear_grads_f64, laplacian_apply_f64, laplacian_f64, laplacian_tangent_f64, model_apply_f64,
                             underflow_eps)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GOLDEN = ["dumbbell_k50_noloop", "dumbbell_k10_loop"]


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


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _golden_graph(mgp, golden, case, dev):
    g = golden(case)
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    return g, mgp.graph.KnnGraph.from_coo(idx, val, g["train_x"].shape[0])


def _knn_graph(mgp, x_np, k, dev):
    x = T(x_np, dev)
    knn = mgp.utils.NearestNeighbors(x)
    D, _ = knn.search(x, k)
    knn.graph(k)
    return knn.knn_graph, D


def _star_ring(mgp, dev, n=12000, hub=3500, seed=11):
    """Node 0 joined to nodes 1..hub (a row of `hub` entries, rows of one entry at the leaves); nodes hub+1..n-1 on a ring (rows
    of two entries)."""
    rng = np.random.default_rng(seed)
    ring = np.arange(hub + 1, n)
    r = np.concatenate([np.zeros(hub, np.int64), np.minimum(ring, np.roll(ring, -1))])
    c = np.concatenate([np.arange(1, hub + 1), np.maximum(ring, np.roll(ring, -1))])
    order = np.lexsort((c, r))
    idx = np.stack([r[order], c[order]])
    val = rng.uniform(0.05, 1.5, idx.shape[1]).astype(np.float32)
    return mgp.graph.KnnGraph.from_coo(T(idx, dev), T(val, dev), n)


# ============================================================================= a. tangent kernel (and the values it differentiates)
def _value_ratio(got, ref, s, f, what):
    """The tangent's form for a value: |got - ref| / (2^-24 scale + floor / 64), which must not exceed 64."""
    assert got.dtype == torch.float64 and bool(torch.isfinite(got).all()), what
    ratio = (got - ref).abs() / (U * s + f / 64.0)
    r = float(ratio.max())
    assert r <= 64.0, (what, r, int(ratio.argmax()))
    return r


def _check_build(data, graph, value, eps32, loops, eid, pad):
    """The six arrays of mgp_laplacian_build (lap_pass) entry by entry against the float64 values `value` that
    laplacian_tangent_f64 returns next to the tangent, in the tangent's form and at its bar: |got - ref| / (2^-24 scale +
    floor / 64) <= 64, scale and floor from oracle/grad_ref.py::laplacian_value_scale_f64.  `vals` is compared at the
    non-padding entries through eid; its padding entries are exactly 0.  Returns the worst ratio."""
    from oracle.grad_ref import laplacian_value_scale_f64
    val, idx = graph.edge_value.double().cpu(), graph.edge_index.cpu()
    value2, scale, floor = laplacian_value_scale_f64(val, idx, graph.n, eps32, loops)
    vals = data.vals.double().cpu()
    assert data.vals.dtype == torch.float32 and bool((vals[pad] == 0).all()), "padding entries of the CSR values must be exactly 0"
    worst = 0.0
    for name in NAMES:
        assert torch.equal(value[name], value2[name])
        if name == "triu":
            got, ref, s, f = vals[~pad], value[name][eid[~pad]], scale[name][eid[~pad]], floor[name][eid[~pad]]
        else:
            got, ref, s, f = getattr(data, name).double().cpu(), value[name], scale[name], floor[name]
        worst = max(worst, _value_ratio(got, ref, s, f, name))
    return worst


def _check_tangent(mgp, graph, eps, loops):
    """Worst ratio |got - ref| / (2^-24 scale + floor / 64) over the six tangent arrays (the bound is 64)."""
    from manifold_gp_amd.graph import LaplacianData
    data = LaplacianData(graph, eps, loops)
    t = data.tangent()
    eps32 = float(np.float32(eps))
    n = graph.n
    val = graph.edge_value.double().cpu()
    idx = graph.edge_index.cpu()
    value, tan, scale, floor = laplacian_tangent_f64(val, idx, n, eps32, loops)
    eid = graph.eid.long().cpu()
    pad = eid < 0
    print("build values n=%d eps=%.4g loops=%s: worst ratio %.2f" % (n, eps32, loops, _check_build(data, graph, value, eps32, loops,
                                                                                               eid, pad)))
    d_vals = t.d_vals.double().cpu()
    assert bool((d_vals[pad] == 0).all()), "padding entries of the tangent CSR must be exactly 0"
    # the CSR's squared distances are the edge list's (the oracle and the kernel read the same numbers)
    assert torch.equal(graph.d2.cpu()[~pad], graph.edge_value.cpu()[eid[~pad]])
    assert int(torch.bincount(eid[~pad], minlength=graph.M).min()) == 2        # every edge in both its rows
    worst = 0.0
    for name in NAMES:
        if name == "triu":
            got, ref, s, f = d_vals[~pad], tan[name][eid[~pad]], scale[name][eid[~pad]], floor[name][eid[~pad]]
        else:
            got, ref, s, f = getattr(t, "d_" + name).double().cpu(), tan[name], scale[name], floor[name]
        assert bool(torch.isfinite(got).all()), name
        ratio = (got - ref).abs() / (U * s + f / 64.0)
        r = float(ratio.max())
        assert r <= 64.0, (name, r, int(ratio.argmax()))
        worst = max(worst, r)
    # the tile-order copy (what the C == 1 / small-C tile kernels stream on a locality-ordered graph) is the same values
    if graph.tiles is not None and graph.tiles.get("rowid") is not None:
        assert torch.equal(t.d_vals_t, t.d_vals.index_select(0, graph.tiles["emap"]))
    return worst


@pytest.mark.parametrize("case", GOLDEN)
@pytest.mark.parametrize("loops,bw", [(lp, b) for lp in (True, False) for b in ("x0.25", "x1", "x4")] + [(True, "underflow")])
def test_tangent_golden_graphs(mgp, golden, dev, case, loops, bw):
    """lap_tangent_pass on the 1,546-node fixtures: every tangent entry within 64 * 2^-24 of its float64 term scale (plus the
    contribution of weights float32 cannot hold as normal numbers).  Bandwidths: the fixture's, a quarter and four times of
    it, and one at which most weights are below 2^-126 (self loops on only: without them D~ could be 0).
    Measured worst ratio: 5.9 of the 64 (x1, k50 fixture); 1.2-1.4 at the underflow bandwidth.
    The values the tangent differentiates (the six arrays of mgp_laplacian_build, _check_build) are held to the same form and
    bar on the same graphs: measured worst 1.90 of the 64 (x4, k10 fixture, no loops)."""
    g, graph = _golden_graph(mgp, golden, case, dev)
    if bw == "underflow":                  # (self loops only: without them an isolated D~ is 0 and the Laplacian undefined)
        eps = underflow_eps(graph.edge_value.double().cpu())
        w = torch.exp(-graph.edge_value.double() / (4 * eps * eps))
        assert float((w < 2.0 ** -126).double().mean()) > 0.5                     # most weights underflow float32
    else:
        eps = float(g["eps"]) * float(bw[1:])
    worst = _check_tangent(mgp, graph, eps, loops)
    print("tangent %s loops=%s %s: worst ratio %.2f" % (case, loops, bw, worst))


@pytest.mark.parametrize("bw", ["x0.25", "x1", "x4", "underflow"])
def test_tangent_star_plus_ring(mgp, dev, bw):
    """One hub row of 3,500 entries (a 16-lane group walks it 219 times) next to rows of one and two entries.
    Measured worst ratio: 14.6 of the 64 (eps x 4); 4.1 at x1, 1.0 at the underflow bandwidth.
    Build values (_check_build; the hub row is 219 steps of lap_pass's float4 / int4 row walk): worst 2.90 of the 64 (x4, no
    loops)."""
    graph = _star_ring(mgp, dev)
    counts = (graph.rowptr[1:] - graph.rowptr[:-1]).cpu()
    nz = torch.bincount(graph.eid.cpu()[graph.eid.cpu() >= 0].long(), minlength=graph.M)
    assert int(nz.min()) == 2
    real = torch.zeros(graph.n, dtype=torch.long).index_add_(0, graph.edge_index[0].cpu(), torch.ones(graph.M, dtype=torch.long))
    real.index_add_(0, graph.edge_index[1].cpu(), torch.ones(graph.M, dtype=torch.long))
    assert int(real.max()) >= 3000 and int((real <= 2).sum()) > 8000 and int(counts.max()) >= 3000
    eps0 = 0.5
    if bw == "underflow":
        eps = underflow_eps(graph.edge_value.double().cpu())
    else:
        eps = eps0 * float(bw[1:])
    worst = _check_tangent(mgp, graph, eps, True)
    worst = max(worst, _check_tangent(mgp, graph, eps, False)) if bw != "underflow" else worst
    print("tangent star+ring %s: worst ratio %.2f" % (bw, worst))


@pytest.fixture(scope="module")
def swiss150k(mgp, dev):
    from tools import synth
    x_np, _ = synth.swiss_roll(150_001, order="random")
    graph, D = _knn_graph(mgp, x_np, 10, dev)
    eps0 = synth.bandwidth_rule(D[:, 1].cpu().numpy(), 0.0)[0]
    return graph, eps0


@pytest.mark.parametrize("bw,loops", [("x1", True), ("x1", False), ("x0.25", True), ("x4", False)])
def test_tangent_past_the_grid_caps(mgp, dev, swiss150k, bw, loops):
    """150,001 rows: past the tangent passes' 65,536-row grid (grid-stride loop) and the backward sums' 131,072; the tiles
    follow a locality order (random point order), so the tile-order copy of the tangent values is checked too.  At a quarter of
    the bandwidth most weights underflow float32.
    Measured worst ratio: 4.2 of the 64 (x4, no loops); 3.8 at x0.25.
    Build values (_check_build; lap_pass's grid covers 65,536 rows, the rest come from its grid-stride loop): worst 2.17 of the
    64 (x0.25)."""
    graph, eps0 = swiss150k
    assert graph.n > 131072 and graph.n > 4096 * 16
    assert graph.tiles is not None and graph.tiles.get("rowid") is not None
    eps = eps0 * float(bw[1:])
    if bw == "x0.25":
        # most weights vanish against the self loop (W < 2^-24: D~ = 1 in float32), a fifth are below 2^-126
        w = torch.exp(-graph.edge_value.double() / (4 * eps * eps))
        assert float((w < U).double().mean()) > 0.5 and float((w < 2.0 ** -126).double().mean()) > 0.1
    worst = _check_tangent(mgp, graph, eps, loops)
    print("tangent swiss150k %s loops=%s: worst ratio %.2f" % (bw, loops, worst))


def _check_edge_values(graph, eps, loops):
    """mgp_edge_values, which = 0 (W), 1 (A), 2 (S) in edge-list order against the float64 values, through the ratio of
    _check_build (same scale, floor and bar).  Returns the worst ratio."""
    from manifold_gp_amd.graph import LaplacianData
    from oracle.grad_ref import laplacian_value_scale_f64
    data = LaplacianData(graph, eps, loops)
    value, scale, floor = laplacian_value_scale_f64(graph.edge_value.double().cpu(), graph.edge_index.cpu(), graph.n,
                                                    float(np.float32(eps)), loops)
    worst = 0.0
    for which, name in enumerate(("w", "a", "triu")):
        out = data.edge_values(which)
        assert out.dtype == torch.float32 and tuple(out.shape) == (graph.M,)
        worst = max(worst, _value_ratio(out.double().cpu(), value[name], scale[name], floor[name], name))
    return worst


@pytest.mark.parametrize("bw", ["x0.25", "x1", "x4", "underflow"])
def test_edge_values_star_plus_ring(mgp, dev, bw):
    """W, A and S per edge on the star-plus-ring graph (the hub's D~ and D are sums of 3,500 terms), with and without self
    loops.  Measured worst ratio: 1.03 of the 64 (underflow bandwidth)."""
    graph = _star_ring(mgp, dev)
    eps = underflow_eps(graph.edge_value.double().cpu()) if bw == "underflow" else 0.5 * float(bw[1:])
    worst = _check_edge_values(graph, eps, True)
    worst = max(worst, _check_edge_values(graph, eps, False)) if bw != "underflow" else worst
    print("edge values star+ring %s: worst ratio %.2f" % (bw, worst))


@pytest.mark.parametrize("bw,loops", [("x1", True), ("x1", False), ("x0.25", True)])
def test_edge_values_at_150k_rows(mgp, dev, swiss150k, bw, loops):
    """The 150,001-row swiss roll: 773,027 edges (1.5 M CSR entries), still UNDER the 8192 x 256 = 2,097,152-thread grid of
    edge_values_kernel (its grid-stride loop is not entered; a graph that enters it needs 2.1 M edges), but every D~ and D it
    reads came from the grid-stride loop of lap_pass.  Measured worst ratio: 1.40 of the 64 (x1, no loops)."""
    graph, eps0 = swiss150k
    assert 700_000 < graph.M < 8192 * 256 and graph.n > 4096 * 16
    worst = _check_edge_values(graph, eps0 * float(bw[1:]), loops)
    print("edge values swiss150k %s loops=%s: worst ratio %.2f" % (bw, loops, worst))


# ============================================================================= b. one fused SpMM, every gradient
COLS = [1, 3, 4, 12, 32, 47, 48, 64, 100, 256, 257, 300]


@pytest.fixture(scope="module")
def spmm_graphs(mgp, dev):
    from tools import synth
    out = {}
    for name, order in (("natural", "morton"), ("ordered", "random")):
        x_np, _ = synth.swiss_roll(6000, seed=3, order=order)
        graph, D = _knn_graph(mgp, x_np, 30, dev)
        eps = synth.bandwidth_rule(D[:, 1].cpu().numpy(), 0.0)[0] * 2.0
        out[name] = (graph, eps)
    return out


def _fused_reference(graph, eps, ops, G):
    """float64 autograd of sum(G . Y), Y = cb base + co post (.) (a xs + b L_sym xs), xs = pre (.) X, and the same expression
    over absolute values (the magnitudes a fp32 evaluation rounds): per-gradient error scales."""
    n = graph.n
    val, idx = graph.edge_value.double().cpu(), graph.edge_index.cpu()
    X, a, b, co, cb, pre, post, base = [o.detach().double().cpu().requires_grad_(True) for o in ops]
    e = torch.tensor(float(np.float32(eps)), dtype=torch.float64, requires_grad=True)
    G = G.double().cpu()
    lap = laplacian_f64(val, idx, n, e, True)
    xs = pre.view(-1, 1) * X
    Y = cb * base + co * post.view(-1, 1) * (a * xs + b * laplacian_apply_f64(lap, idx, xs))
    ref = torch.autograd.grad((G * Y).sum(), [X, e, a, b, co, cb, pre, post, base])
    # scales: the same expression on |operands| with |L| = diag + S + S^T; eps through |L'| = |tangent| + term scale
    Xa, aa, ba, coa, cba, prea, posta, basea = [o.detach().abs().requires_grad_(True) for o in (X, a, b, co, cb, pre, post, base)]
    lv = laplacian_f64(val, idx, n, e.detach(), True)
    labs = dict(lv, diag=lv["diag"].abs())
    r, c = idx[0].long(), idx[1].long()

    def absL(M, d, s):
        return d.view(-1, 1) * M + torch.zeros_like(M).index_add(0, r, s.view(-1, 1) * M[c]) \
            + torch.zeros_like(M).index_add(0, c, s.view(-1, 1) * M[r])
    xsa = prea.view(-1, 1) * Xa
    Ya = cba * basea + coa * posta.view(-1, 1) * (aa * xsa + ba * absL(xsa, labs["diag"], labs["triu"]))
    sc = list(torch.autograd.grad((G.abs() * Ya).sum(), [Xa, aa, ba, coa, cba, prea, posta, basea]))
    _, tan, tscale, _ = laplacian_tangent_f64(val, idx, n, float(np.float32(eps)), True)
    h = (G.abs() * coa.detach() * posta.detach().view(-1, 1))
    dl = absL(xsa.detach(), tan["diag"].abs() + tscale["diag"], tan["triu"].abs() + tscale["triu"])
    seps = ba.detach() * (h * dl).sum()
    scales = [sc[0], seps] + sc[1:]
    return [x.detach() for x in ref], [s.detach() for s in scales]


@pytest.mark.parametrize("order", ["natural", "ordered"])
@pytest.mark.parametrize("fused_sums", [True, False])
@pytest.mark.parametrize("C", COLS)
def test_fused_spmm_all_gradients(mgp, dev, spmm_graphs, order, fused_sums, C):
    """autograd.fused_spmm with every tensor argument requiring grad: the nine gradients (X, eps, a, b, co, cb, pre, post, base)
    against float64 autograd of the same expression.  Bound per entry: |got - ref| <= 2e-5 * (the same gradient over absolute
    values); where |ref| is at least a tenth of that scale also <= 2e-3 |ref|.  (With random-sign operands a gradient that is a
    sum of K products is ~K^-1/2 of that scale -- 1/500 for the eps gradient here -- so the bound must sit well under 1e-3 of it
    to see an O(1) error: taking L xs for L' xs moves the eps gradient by 2.2e-4 of its scale.)
    C > 256 runs in 256-column chunks; C >= 48 on the natural-order graph runs the matrix-core kernel forward and a gather
    kernel on the tangent CSR (it carries no matrix-core image); the ordered graph streams the tile-order copies (vals_t,
    d_vals_t).
    Measured worst ratio: 0.033 of the 2e-5 bound."""
    from manifold_gp_amd import _lib, autograd
    from manifold_gp_amd.graph import LaplacianData
    graph, eps = spmm_graphs[order]
    n = graph.n
    data = LaplacianData(graph, eps, True)
    lib = _lib.lib()
    if order == "ordered":
        assert graph.tiles is not None and graph.tiles.get("rowid") is not None
    else:
        assert graph.tiles is None or graph.tiles.get("rowid") is None
        if 48 <= C <= 256:
            assert lib.mgp_spmm_kernel_choice(ctypes.byref(data.csr(wide=True)), C, 0, 0) == 3
            t = data.tangent()
            assert lib.mgp_spmm_kernel_choice(ctypes.byref(graph.csr_with(t.d_vals, t.d_diag, t.d_vals_t)), C, 0, 0) != 3
    gen = torch.Generator().manual_seed(1000 + C)

    def rnd(*shape, lo=None):
        v = torch.randn(*shape, generator=gen)
        return (v.abs() + lo if lo is not None else v).to(dev)
    X, G, base = rnd(n, C), rnd(n, C), rnd(n, C)
    pre, post = rnd(n, lo=0.5), rnd(n, lo=0.5)
    a, b, co, cb = (torch.tensor(v, device=dev) for v in (0.37, 1.3, 0.8, -0.6))
    ops = [X, a, b, co, cb, pre, post, base]
    leaves = [o.clone().requires_grad_(True) for o in ops]
    e = torch.tensor(float(eps), device=dev, requires_grad=True)
    old = autograd.FUSED_BACKWARD_SUMS[0]
    autograd.FUSED_BACKWARD_SUMS[0] = fused_sums
    try:
        Xl, al, bl, col, cbl, prel, postl, basel = leaves
        Y = autograd.fused_spmm(data, Xl, e, al, bl, col, cbl, prel, postl, basel)
        got = torch.autograd.grad((G * Y).sum(), [Xl, e, al, bl, col, cbl, prel, postl, basel])
    finally:
        autograd.FUSED_BACKWARD_SUMS[0] = old
    ref, scales = _fused_reference(graph, eps, ops, G)
    names = ["X", "eps", "a", "b", "co", "cb", "pre", "post", "base"]
    worst = 0.0
    for name, x, r, s in zip(names, got, ref, scales):
        x = x.detach().double().cpu().reshape(r.shape)
        err = (x - r).abs()
        s = s.reshape(r.shape)
        assert bool((err <= 2e-5 * s).all()), (name, float((err / s).max()))
        big = r.abs() >= 0.1 * s
        assert bool((err[big] <= 2e-3 * r.abs()[big]).all()), (name, float((err[big] / r.abs()[big]).max()))
        worst = max(worst, float((err / (2e-5 * s)).max()))
    print("fused_spmm %s sums=%s C=%d: worst ratio %.2e" % (order, fused_sums, C, worst))


# ============================================================================= c. mgp_spmm_backward_sums directly
INPUTS = ("h", "dlx", "xs", "gxs", "X", "g", "lx")


def _legal(p):
    """The null-input rules of mgp_spmm_backward_sums (include/mgp_hip.h)."""
    if p["gpre"] and not (p["gxs"] and p["X"]):
        return False
    if p["gpost"] and not (p["g"] and p["xs"] and p["lx"]):
        return False
    if p["dlx"] and not p["h"]:
        return False
    return True


def _sums_ref(arr, p, av, bv, cov, n, step=65536):
    """float64 numpy: <h, dlx>, <h, xs>, gpre, gpost and their magnitude sums, chunked over rows."""
    s = np.zeros(2)
    m = np.zeros(2)
    gpre = np.zeros(n) if p["gpre"] else None
    gpost = np.zeros(n) if p["gpost"] else None
    mpre = np.zeros(n) if p["gpre"] else None
    mpost = np.zeros(n) if p["gpost"] else None
    for r0 in range(0, n, step):
        b = {k: (arr[k][r0:r0 + step].astype(np.float64) if p[k] else None) for k in INPUTS}
        if p["dlx"]:
            t = b["h"] * b["dlx"]
            s[0] += t.sum()
            m[0] += np.abs(t).sum()
        if p["h"] and p["xs"]:
            t = b["h"] * b["xs"]
            s[1] += t.sum()
            m[1] += np.abs(t).sum()
        if p["gpre"]:
            t = b["gxs"] * b["X"]
            gpre[r0:r0 + step] = t.sum(1)
            mpre[r0:r0 + step] = np.abs(t).sum(1)
        if p["gpost"]:
            t = b["g"] * (av * b["xs"] + bv * b["lx"])
            gpost[r0:r0 + step] = cov * t.sum(1)
            mpost[r0:r0 + step] = abs(cov) * (np.abs(b["g"]) * (abs(av) * np.abs(b["xs"]) + abs(bv) * np.abs(b["lx"]))).sum(1)
    return s, m, gpre, gpost, mpre, mpost


def _patterns():
    for bits in itertools.product([0, 1], repeat=len(INPUTS) + 2):
        yield dict(zip(INPUTS + ("gpre", "gpost"), bits))


def _run_sums(lib, dev, n, C, arr_dev, p, av, bv, cov):
    from manifold_gp_amd._lib import ptr, stream
    nb = lib.mgp_spmm_backward_blocks(n)
    part = torch.full((nb, 2), float("nan"), dtype=torch.float32, device=dev)
    gpre = torch.full((n,), float("nan"), dtype=torch.float32, device=dev) if p["gpre"] else None
    gpost = torch.full((n,), float("nan"), dtype=torch.float32, device=dev) if p["gpost"] else None
    rc = lib.mgp_spmm_backward_sums(n, C, *[ptr(arr_dev[k] if p[k] else None) for k in INPUTS], float(av), float(bv), float(cov),
                                    ptr(part), ptr(gpre), ptr(gpost), stream())
    return rc, part, gpre, gpost


@pytest.mark.parametrize("n", [1, 255, 257, 131072, 131073, 300007])
@pytest.mark.parametrize("C", [1, 5, 12, 64, 300])
def test_backward_sums_kernel_vs_float64(mgp, dev, n, C):
    """mgp_spmm_backward_sums against float64 numpy at row counts around one workgroup (256 rows) and the 512 x 256 = 131,072
    rows of its grid (the grid-stride loop).  At n <= 257, C <= 12 every legal pattern of null inputs / outputs (135) runs and
    each illegal one (377) returns MGP_ERR_ARG; at the other shapes the 33 patterns with everything on or with only the eps / a
    reductions (what autograd._FusedSpmm.backward issues), with every mix of the unused inputs.
    Bound: a recursive fp32 sum of K products is within K 2^-24 of the sum of their magnitudes; a thread sums C ceil(n /
    131072) products per scalar, the block and the caller add 512 + 32 more levels: |got - ref| <= 2^-24 (C ceil(n / 131072)
    + 576) * sum |terms| for the two scalars, (C + 3) 2^-24 * sum_c |terms| per row for gpre / gpost (C fused multiply-adds,
    b lx, cov p).
    Measured worst ratio: 0.86 (n = 300,007, C = 1); at C = 300 0.02."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    nb = lib.mgp_spmm_backward_blocks(n)
    assert nb == min(512, -(-n // 256))
    if n > 131072:
        assert nb * 256 < n                           # the grid-stride loop is what covers the rows past the grid
    gen = torch.Generator(device=dev).manual_seed(n * 7 + C)
    arr_dev = {k: torch.randn(n, C, generator=gen, device=dev) for k in INPUTS}
    arr = {k: v.cpu().numpy() for k, v in arr_dev.items()}
    av, bv, cov = (float(np.float32(v)) for v in (0.37, -1.3, 0.8))      # the values the kernel receives
    small = n <= 257 and C <= 12
    pats = list(_patterns())
    legal = [p for p in pats if _legal(p)]
    if not small:
        # at the large shapes: the patterns autograd._FusedSpmm.backward issues, and everything on
        legal = [p for p in legal if all(p.values()) or (p["dlx"] and p["h"] and p["xs"] and not p["gpre"] and not p["gpost"])
                 or (p["h"] and p["xs"] and not p["dlx"] and not p["gpre"] and not p["gpost"])]
    worst = 0.0
    for p in legal:
        rc, part, gpre, gpost = _run_sums(lib, dev, n, C, arr_dev, p, av, bv, cov)
        assert rc == 0, p
        s, m, rpre, rpost, mpre, mpost = _sums_ref(arr, p, av, bv, cov, n)
        tot = part.double().sum(0).cpu().numpy()
        k = C * -(-n // 131072) + 576
        err = np.abs(tot - s)
        assert (err <= k * U * m).all(), (p, tot, s, m)
        worst = max(worst, float((err / np.maximum(k * U * m, 1e-300)).max()))
        for got, ref, mag in ((gpre, rpre, mpre), (gpost, rpost, mpost)):
            if got is None:
                continue
            e = np.abs(got.double().cpu().numpy() - ref)
            assert (e <= (C + 3) * U * mag).all(), (p, float((e / np.maximum((C + 3) * U * mag, 1e-300)).max()))
            worst = max(worst, float((e / np.maximum((C + 3) * U * mag, 1e-300)).max()))
    if small:
        for p in pats:
            if not _legal(p):
                rc, _, _, _ = _run_sums(lib, dev, n, C, arr_dev, p, av, bv, cov)
                assert rc == -1, p                     # MGP_ERR_ARG
    from manifold_gp_amd._lib import ptr, stream
    part = torch.empty(max(nb, 1), 2, device=dev)
    h = arr_dev["h"]
    assert lib.mgp_spmm_backward_sums(n, C, ptr(h), None, None, None, None, None, None, 0.0, 0.0, 0.0, None, None, None,
                                      stream()) == -1  # no partials
    assert lib.mgp_spmm_backward_sums(0, C, ptr(h), None, None, None, None, None, None, 0.0, 0.0, 0.0, ptr(part), None, None,
                                      stream()) == -1
    assert lib.mgp_spmm_backward_sums(n, 0, ptr(h), None, None, None, None, None, None, 0.0, 0.0, 0.0, ptr(part), None, None,
                                      stream()) == -1
    print("backward_sums n=%d C=%d: %d patterns, worst ratio %.3f" % (n, C, len(legal), worst))


# ============================================================================= d. operator-level gradients
def check_theta(got, ref, scale, names):
    """The operator-level bound: |got - ref| <= 2e-4 scale; where |ref| >= scale / 10 also <= 2e-3 |ref|.  Returns the worst
    ratio error / (2e-4 scale)."""
    worst = 0.0
    for nm, x, r, s in zip(names, got, ref, scale):
        if s == 0.0:
            assert x == 0.0 or abs(x) <= 1e-30, (nm, x)
            continue
        assert abs(x - r) <= 2e-4 * s, (nm, x, r, s)
        if abs(r) >= 0.1 * s:
            assert abs(x - r) <= 2e-3 * abs(r), (nm, x, r)
        worst = max(worst, abs(x - r) / (2e-4 * s))
    return worst


@pytest.mark.parametrize("case", GOLDEN)
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("norm,nu", [(nm, v) for nm in ("symmetric", "randomwalk") for v in (1, 2, 3)] + [("randomwalk_T", 1)])
@pytest.mark.parametrize("C", [1, 12, 32, 64])
def test_operator_gradients_vs_float64(mgp, golden, dev, case, loops, norm, nu, C):
    """<W, Q3 V> with Q3 = Noise(Scale(Precision(L))) (for the transposed random walk: <W, L^T V>, the precision ignores the
    transpose) and its gradients wrt eps, lengthscale, outputscale, noise and V against oracle/grad_ref.py::model_apply_f64.
    Bound per hyper-parameter: |got - ref| <= 2e-4 sum_i |W_i| |(dQ3/d theta V)_i| (float64), and <= 2e-3 |ref| where |ref| is a
    tenth of that scale or more; V: |got - ref| <= 2e-4 (|Q3| |W|) entrywise bound by max |ref| (Q3 = Q3^T).
    Measured worst ratio: 9.6e-5 of the hyper-parameter bound; V: 7.7e-7 of max |ref|."""
    O = mgp.operators
    g = golden(case)
    n = g["train_x"].shape[0]
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    gen = torch.Generator().manual_seed(31 * C + nu)
    V64 = torch.randn(n, C, generator=gen, dtype=torch.float64)
    W64 = torch.randn(n, C, generator=gen, dtype=torch.float64)
    theta = [float(g["eps"]), float(g["kappa"]), 0.7, 1e-3]
    th = [torch.tensor(v, device=dev, requires_grad=True) for v in theta]
    V = V64.float().to(dev).requires_grad_(True)
    W = W64.float().to(dev)
    nrm = "randomwalk" if norm == "randomwalk_T" else norm
    lap = O.GraphLaplacianOperator(val, idx, n, th[0].view(1, 1), nrm, loops, norm == "randomwalk_T")
    if norm == "randomwalk_T":
        out = lap.matmul(V)
        stop, used = "L", [0]
    else:
        out = O.NoiseWrapperOperator(O.ScaleWrapperOperator(O.PrecisionMaternOperator(lap, nu, th[1]), th[2]), th[3]).matmul(V)
        stop, used = "Q3", [0, 1, 2, 3]
    loss = (W * out).sum()
    gr = torch.autograd.grad(loss, [th[i] for i in used] + [V])
    got = np.array([float(x) for x in gr[:-1]])
    th32 = [float(np.float32(v)) for v in theta]
    val64, idx64 = torch.from_numpy(g["edge_value"].astype(np.float64)), torch.from_numpy(g["edge_index"].astype(np.int64))
    W32, V32 = W.double().cpu(), V.detach().double().cpu()
    ref, scale = bilinear_grads_f64(val64, idx64, n, th32, nu, nrm, loops, V32, W32, norm == "randomwalk_T", stop)
    worst = check_theta(got, ref[used], scale[used], ["eps", "kappa", "outputscale", "noise"][:len(used)])
    # V: the gradient is A^T W
    Vl = V32.clone().requires_grad_(True)
    thl = [torch.tensor(v, dtype=torch.float64) for v in th32]
    refV = torch.autograd.grad((W32 * model_apply_f64(val64, idx64, n, *thl, nu, nrm, loops, Vl, transposed=norm == "randomwalk_T",
                                                      stop=stop)).sum(), Vl)[0]
    eV = float((gr[-1].double().cpu() - refV).abs().max())
    assert eV <= 2e-4 * float(refV.abs().max()), (eV, float(refV.abs().max()))
    print("operator %s loops=%s %s nu=%d C=%d: worst theta ratio %.2e, V rel %.1e" % (case, loops, norm, nu, C, worst,
                                                                                    eV / float(refV.abs().max())))
