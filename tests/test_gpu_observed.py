"""Posterior on a subset of nodes with per-node noise on the MI355X (operator form 3, A = diag(w) + s Q2): the apply in every
SpMM kernel family against float64 and bit for bit against form 2 at w = 1, the Jacobi diagonal, the CG contract, the
refused paths, samples and means against a dense float64 oracle fed the same noise, sample statistics, the public methods
and the 60k graph."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _observed_ref as ref
from _sampling_ref import edge_factor, edge_noise, node_noise

pytestmark = pytest.mark.gpu

NORMS = ["symmetric", "randomwalk"]


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


def _desc(mgp, g, dev, norm, nu, scale=0.8):
    idx = T(g["edge_index"].astype(np.int64), dev)
    val = T(g["edge_value"], dev)
    eps = torch.tensor([[float(g["eps"])]], device=dev)
    lap = mgp.operators.GraphLaplacianOperator(val, idx, g["train_x"].shape[0], eps, norm, bool(g["self_loops"]))
    kappa = torch.tensor([[float(g["kappa"])]], device=dev)
    return mgp.operators.PrecisionMaternOperator(lap, nu, kappa)._descriptor().with_(scale=scale)


def _weights(n, dev, seed=0):
    """random non-negative weights with zeros (about a third)"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.05, 1.0, n) * (rng.random(n) > 0.33)
    return T(w.astype(np.float32), dev)


@pytest.fixture(autouse=True)
def _restore_switches(mgp):
    yield
    lib = mgp._lib.lib()
    lib.mgp_spmm_set_tile_mode(1)
    lib.mgp_spmm_set_tile_small_mode(1)
    lib.mgp_spmm_set_tile_wide_mode(1)
    lib.mgp_spmm_set_dict_mode(1)
    lib.mgp_spmm_set_v4_mode(1)
    lib.mgp_spmm_set_mt_mode(1)


# mode name -> (tile, tile_small, tile_wide, dict, v4, mt)
MODES = {
    "production": (1, 1, 1, 1, 1, 1),
    "gather": (0, 0, 0, 0, 0, 0),            # spmv_kernel (C = 1), spmm_row16_kernel (C <= 16), spmm_kernel
    "v4": (0, 0, 0, 0, 2, 0),                # spmm_v4_kernel for C > 16
    "wide": (1, 1, 2, 0, 1, 0),              # spmm_tile_wide_kernel (chunked dictionary)
    "dict": (1, 1, 1, 2, 1, 0),              # spmm_dict_kernel (lanes over columns)
}


def _set_mode(lib, mode):
    t, ts, tw, dc, v4, mt = MODES[mode]
    lib.mgp_spmm_set_tile_mode(t)
    lib.mgp_spmm_set_tile_small_mode(ts)
    lib.mgp_spmm_set_tile_wide_mode(tw)
    lib.mgp_spmm_set_dict_mode(dc)
    lib.mgp_spmm_set_v4_mode(v4)
    lib.mgp_spmm_set_mt_mode(mt)


def _family(lib, desc, C, mode):
    """(kernel choice, gather variant) of the chain's launches for this descriptor / width"""
    csr = desc.struct(wide=C >= 48).L
    choice = lib.mgp_spmm_kernel_choice(ctypes.byref(csr), C, 0, 0)
    if choice != 0:
        return choice, None
    return choice, ("spmv" if C == 1 else "row16" if C <= 16 and C % 4 == 0 else "v4" if MODES[mode][4] == 2 else "gather")


# ------------------------------------------------------------------------------------------------ 1 + 2: the apply
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_form3_apply_vs_fp64_and_bitwise_form2(mgp, golden, dev, norm, nu):
    lib = mgp._lib.lib()
    g = golden("dumbbell_k10_loop")
    desc = _desc(mgp, g, dev, norm, nu)
    n, s = desc.n, 3e-2
    w = _weights(n, dev, nu)
    Q2 = ref.device_q2(desc)
    orders = [("natural", desc)]
    rdesc, rg = desc.relabelled()
    if rdesc is not None:
        orders.append(("locality", (rdesc, rg)))
    seen = set()
    wn = w.double().cpu().numpy()
    for C in (1, 4, 12, 16, 32, 64, 128, 256):
        X = torch.randn(n, C, device=dev)
        Xn = X.double().cpu().numpy()
        want = wn[:, None] * Xn + s * (Q2 @ Xn)
        scale = np.abs(wn)[:, None] * np.abs(Xn) + s * (abs(Q2) @ np.abs(Xn))
        for mode in MODES:
            _set_mode(lib, mode)
            for oname, od in orders:
                if oname == "natural":
                    d3, d2, Xo = desc.with_(form=3, noise=s, obs_w=w), desc.with_(form=2, noise=s), X
                else:
                    rd, rgr = od
                    d3, d2, Xo = rd.with_(form=3, noise=s, obs_w=rel_w(rd, desc, w)), rd.with_(form=2, noise=s), rgr.permute(X)
                seen.add((C,) + _family(lib, d3, C, mode))
                Y3 = _struct_apply(lib, d3, Xo)
                Y2 = _struct_apply(lib, d2, Xo)
                Y1 = _struct_apply(lib, d3.with_(obs_w=torch.ones_like(w) if oname == "natural" else rel_w(rd, desc, torch.ones_like(w))), Xo)
                if oname != "natural":
                    Y3, Y2, Y1 = rgr.unpermute(Y3), rgr.unpermute(Y2), rgr.unpermute(Y1)
                err = (np.abs(Y3.double().cpu().numpy() - want) / scale.clip(1e-30)).max()
                assert err < 2e-6 * (nu + 1), (C, mode, oname, err)
                # w = 1 rides the same epilogue as form 2: bit for bit
                assert torch.equal(Y1, Y2), (C, mode, oname)
    kinds = {k[1:] for k in seen}
    for want_kind in [(0, "spmv"), (0, "row16"), (0, "v4"), (0, "gather"), (1, None), (2, None), (5, None), (6, None)]:
        assert want_kind in kinds, (want_kind, sorted(seen, key=str))


def rel_w(rdesc, desc, w):
    """obs_w as Descriptor.relabelled() carries it"""
    return desc.with_(form=3, obs_w=w).relabelled()[0].obs_w


def _struct_apply(lib, d, X):
    """one mgp_operator_apply on the descriptor's own CSR (no relabelling inside): kernel choice as the switches say"""
    from manifold_gp_amd import _lib
    C = X.shape[1]
    op = d.struct(wide=C >= 48)
    Y = torch.empty_like(X)
    wb = lib.mgp_operator_workspace_bytes(ctypes.byref(op), C)
    work = torch.empty(wb, dtype=torch.uint8, device=X.device)
    _lib.check(lib.mgp_operator_apply(ctypes.byref(op), _lib.ptr(X), C, _lib.ptr(Y), _lib.ptr(work), wb, _lib.stream()),
               "mgp_operator_apply")
    return Y


def _curve_desc(mgp, dev, norm, nu, n0=8192, k=12, shuffle=False, seed=5):
    """descriptor on a k-NN graph of n0 points along a 3-d curve (tests/test_gpu_parity.py::test_spmm_matrix_core_tiles):
    n0 >= graph.MT_MIN_NODES, so that the wide CSR carries the matrix-core tile image; shuffle: nodes without locality (the
    solvers then iterate on the relabelled copy)"""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.random(n0))
    x = np.stack([np.cos(6.28 * t) * (1 + t), np.sin(6.28 * t) * (1 + t), 0.3 * np.sin(40 * t)], 1).astype(np.float32)
    if shuffle:
        x = x[rng.permutation(n0)]
    nn = mgp.utils.NearestNeighbors(T(x, dev))
    idx, val = nn.graph(k)
    lap = mgp.operators.GraphLaplacianOperator(val, idx, n0, torch.tensor([[0.1]], device=dev), norm, graph=nn.knn_graph)
    return mgp.operators.PrecisionMaternOperator(lap, nu, torch.tensor([[0.5]], device=dev))._descriptor().with_(scale=0.8)


@pytest.mark.parametrize("norm", NORMS)
def test_form3_matrix_core_kernel(mgp, dev, norm):
    """48 <= C <= 256 on the matrix cores: spmm_mt_cbv_kernel (PRE = false / true) against float64 and, at w = 1, bit for bit
    against form 2 on spmm_mt_kernel; the choice is asserted.  Also through Descriptor.apply, the production wide path."""
    from manifold_gp_amd.graph import MT_MIN_NODES
    lib = mgp._lib.lib()
    desc = _curve_desc(mgp, dev, norm, 2)
    assert desc.n >= MT_MIN_NODES
    rd, _ = desc.relabelled(wide=True)
    d = rd if rd is not None else desc             # the matrix the wide products run on (the image lives there)
    n, s = d.n, 5e-2
    w = _weights(n, dev, 7)
    Q2 = ref.device_q2(d)
    wn = w.double().cpu().numpy()
    for C in (48, 64, 128, 256):
        d3 = d.with_(form=3, noise=s, obs_w=w)
        csr = d3.struct(wide=True).L
        assert lib.mgp_spmm_kernel_choice(ctypes.byref(csr), C, 0, 0) == 3, C
        X = torch.randn(n, C, device=dev)
        Xn = X.double().cpu().numpy()
        want = wn[:, None] * Xn + s * (Q2 @ Xn)
        scale = np.abs(wn)[:, None] * np.abs(Xn) + s * (abs(Q2) @ np.abs(Xn))
        Y3 = _struct_apply(lib, d3, X)
        assert (np.abs(Y3.double().cpu().numpy() - want) / scale).max() < 6e-6, C
        Y1 = _struct_apply(lib, d.with_(form=3, noise=s, obs_w=torch.ones_like(w)), X)
        assert torch.equal(Y1, _struct_apply(lib, d.with_(form=2, noise=s), X)), C
        # the same family with the image switched off (gather kernels) agrees to rounding
        lib.mgp_spmm_set_mt_mode(0)
        assert lib.mgp_spmm_kernel_choice(ctypes.byref(csr), C, 0, 0) != 3
        Yg = _struct_apply(lib, d3, X)
        lib.mgp_spmm_set_mt_mode(1)
        assert (np.abs(Yg.double().cpu().numpy() - want) / scale).max() < 6e-6, C
    # Descriptor.apply in the caller's order (permutes obs_w with the chain order where there is one)
    wc = _weights(desc.n, dev, 8)
    X = torch.randn(desc.n, 64, device=dev)
    Q2c = ref.device_q2(desc)
    Xn = X.double().cpu().numpy()
    want = wc.double().cpu().numpy()[:, None] * Xn + s * (Q2c @ Xn)
    scale = np.abs(wc.double().cpu().numpy())[:, None] * np.abs(Xn) + s * (abs(Q2c) @ np.abs(Xn))
    Y = desc.with_(form=3, noise=s, obs_w=wc).apply(X)
    assert (np.abs(Y.double().cpu().numpy() - want) / scale).max() < 6e-6


def test_reference_matrix_matches_oracle(mgp, golden, dev):
    """The float64 Q2 the apply / CG tests build from the library's CSR (tests/_observed_ref.py::device_q2) is the oracle's
    dense Matern precision (oracle/laplacian.py, oracle/precision.py::dense_matern_precision) to fp32 rounding of the values,
    and the form-3 apply agrees with the oracle directly."""
    from oracle.precision import dense_matern_precision
    g = golden("dumbbell_k10_loop")
    for norm in NORMS:
        for nu in (1, 2, 3):
            desc = _desc(mgp, g, dev, norm, nu)
            lo = ref.oracle(g, norm)
            Qo = 0.8 * dense_matern_precision(lo.dense(), nu, float(g["kappa"]), lo.degree if norm == "randomwalk" else None)
            Qd = ref.device_q2(desc).toarray()
            assert np.abs(Qd - Qo).max() <= 1e-5 * np.abs(Qo).max(), (norm, nu)
            w = _weights(desc.n, dev, nu)
            X = torch.randn(desc.n, 4, device=dev)
            Y = desc.with_(form=3, noise=3e-2, obs_w=w).apply(X).double().cpu().numpy()
            Xn = X.double().cpu().numpy()
            want = w.double().cpu().numpy()[:, None] * Xn + 3e-2 * (Qo @ Xn)
            assert np.abs(Y - want).max() <= 2e-5 * np.abs(want).max(), (norm, nu)


# ------------------------------------------------------------------------------------------------ 3: Jacobi
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_form3_jacobi(mgp, golden, dev, norm, nu):
    g = golden("dumbbell_k10_loop")
    desc = _desc(mgp, g, dev, norm, nu)
    s = 2e-2
    w = _weights(desc.n, dev, 11)
    m3 = desc.with_(form=3, noise=s, obs_w=w).jacobi().double().cpu().numpy()
    q = 1.0 / desc.jacobi().double().cpu().numpy()                 # form 0: q_i as the kernel computes it
    want = 1.0 / (w.double().cpu().numpy() + s * q)
    assert np.allclose(m3, want, rtol=2e-6, atol=0), np.abs(m3 / want - 1).max()
    if nu <= 2:                                                      # exact for nu <= 2
        d = ref.device_q2(desc).diagonal()
        assert np.allclose(m3, 1.0 / (w.double().cpu().numpy() + s * d), rtol=1e-5)


# ------------------------------------------------------------------------------------------------ 4: the CG contract
def _true_rel(A, X, B):
    X, B = np.asarray(X, np.float64), np.asarray(B, np.float64)
    return np.linalg.norm(B - A @ X, axis=0) / np.linalg.norm(B, axis=0)


@pytest.mark.parametrize("norm,nu,C", [("randomwalk", 2, 1), ("symmetric", 2, 1), ("randomwalk", 3, 4), ("symmetric", 1, 16)])
def test_form3_cg_contract(mgp, golden, dev, norm, nu, C):
    from manifold_gp_amd.solvers import CgPlan
    g = golden("dumbbell_k10_loop")
    desc = _desc(mgp, g, dev, norm, nu)
    n, s = desc.n, 1e-2
    w = _weights(n, dev, 3)
    d3 = desc.with_(form=3, noise=s, obs_w=w)
    Q2 = ref.device_q2(desc)
    import scipy.sparse as sp
    A3 = sp.diags(w.double().cpu().numpy()) + s * Q2
    B = torch.randn(n, C, device=dev)
    Bn = B.double().cpu().numpy()
    # stop rule and an honest resid
    tol = 1e-4
    # fp32 floor of the true residual (tests/test_gpu_solver_contract.py): F_c = 4 eps32 ||A||_2 ||x_c|| / ||b_c||
    norm_a = float(np.linalg.eigvalsh(A3.toarray()).max())

    def floor(X):
        return 4 * 2.0 ** -23 * norm_a * np.linalg.norm(X, axis=0) / np.linalg.norm(Bn, axis=0)
    plan = CgPlan(d3, C, tol=tol, stop_mode=1, max_iter=5000)
    assert not plan.complex_shift
    X = plan.solve(B).double().cpu().numpy()
    true = _true_rel(A3, X, Bn)
    assert plan.status == 1 and max(plan.resid) <= tol, (plan.status, plan.resid)
    assert (true <= 2 * tol + floor(X)).all(), (true, floor(X))
    assert (true <= 2 * np.array(plan.resid) + floor(X)).all(), (true, plan.resid)
    its = plan.iters
    plan.close()
    # the max_iter exit reports the residual it stopped at
    plan = CgPlan(d3, C, tol=1e-12, stop_mode=1, max_iter=5)
    X = plan.solve(B).double().cpu().numpy()
    true = _true_rel(A3, X, Bn)
    assert plan.status == 2 and plan.iters == 5 and its > 5
    assert (true <= 2 * np.array(plan.resid) + floor(X)).all() and (np.array(plan.resid) <= 2 * true + floor(X)).all()
    plan.close()
    # refinement down to 1e-7 on the float64 true residual (mgp_operator_apply_f64 on form 3)
    plan = CgPlan(d3, C, tol=1e-7, stop_mode=1, max_iter=5000, refine=4)
    plan.solve(B)
    x64 = plan.solution64_view().cpu().numpy()
    assert plan.status == 1 and _true_rel(A3, x64, Bn).max() <= 2e-7, _true_rel(A3, x64, Bn)
    # rebind: new weights of the same structure
    w2 = _weights(n, dev, 4)
    assert plan.rebind(desc.with_(form=3, noise=2 * s, obs_w=w2))
    plan.solve(B)
    A3b = sp.diags(w2.double().cpu().numpy()) + 2 * s * Q2
    assert plan.status == 1 and _true_rel(A3b, plan.solution64_view().cpu().numpy(), Bn).max() <= 2e-7
    # obs_w appears / disappears: another structure (form 2 <-> 3), a new plan
    assert not plan.rebind(desc.with_(form=2, noise=s))
    plan.close()
    p2 = CgPlan(desc.with_(form=2, noise=s), C, tol=1e-4, stop_mode=1, max_iter=5000)
    assert not p2.rebind(d3)
    p2.close()


def test_form3_plan_cache_keys(mgp, golden, dev):
    from manifold_gp_amd import solvers
    g = golden("dumbbell_k10_loop")
    desc = _desc(mgp, g, dev, "randomwalk", 2)
    s = 1e-2
    w, w2 = _weights(desc.n, dev, 1), _weights(desc.n, dev, 2)
    kw = dict(tol=1e-5, stop_mode=1, max_iter=5000)
    solvers.clear_plan_cache()
    p3 = solvers._cached_plan(desc.with_(form=3, noise=s, obs_w=w), 1, kw)
    p2 = solvers._cached_plan(desc.with_(form=2, noise=s), 1, kw)
    assert p3 is not p2
    assert solvers._cached_plan(desc.with_(form=3, noise=s, obs_w=w2), 1, kw) is p3      # rebound: new weights, same plan
    assert p3._vkey[-1] == w2.data_ptr()
    # the solve through the cache sees the new weights
    B = torch.randn(desc.n, 1, device=dev)
    X = solvers.cg_solve(desc.with_(form=3, noise=s, obs_w=w2), B, **kw)[0]
    import scipy.sparse as sp
    A3 = sp.diags(w2.double().cpu().numpy()) + s * ref.device_q2(desc)
    assert _true_rel(A3, X.double().cpu().numpy(), B.double().cpu().numpy()).max() <= 2e-5
    solvers.clear_plan_cache()


# ------------------------------------------------------------------------------------------------ 5: refused paths
def test_form3_refused_by_partitioned_and_distributed_paths(mgp, golden, dev):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    g = golden("dumbbell_k10_loop")
    desc = _desc(mgp, g, dev, "symmetric", 2)
    n = desc.n
    w = _weights(n, dev, 5)
    op = desc.with_(form=3, noise=1e-2, obs_w=w).struct()
    X = torch.randn(n, 1, device=dev)
    Y = torch.empty_like(X)
    work = torch.empty(4 * n * 4 + 4096, dtype=torch.uint8, device=dev)
    # a stand-in for an RCCL communicator: it is never dereferenced.  All three entry points refuse form 3 before any
    # collective (operator.hip mgp_operator_apply_dist, cg.hip plan_create_impl, pcg.hip mgp_pcg_plan_create check the form
    # first); the int it points at lives as long as the test
    fake = ctypes.c_int(0)
    dummy_comm = ctypes.c_void_p(ctypes.addressof(fake))
    assert lib.mgp_operator_apply_part(ctypes.byref(op), dummy_comm, 0, 1, _lib.ptr(X), 1, _lib.ptr(Y), _lib.ptr(work),
                                       work.numel(), _lib.stream()) == -3
    prm = _lib.CgParamsT(1e-5, 100, 0, 1, 0, 1, 0)
    handle = ctypes.c_void_p(0)
    assert lib.mgp_cg_plan_create_dist(ctypes.byref(op), 1, None, ctypes.byref(prm), dummy_comm, 0, 1, _lib.ptr(work),
                                       work.numel(), _lib.stream(), ctypes.byref(handle)) == -3
    rows = (ctypes.c_int64 * 2)(n, n)
    assert lib.mgp_pcg_plan_create(ctypes.byref(op), rows, 0, n, n, dummy_comm, 0, 1, None, 0, ctypes.byref(prm),
                                   _lib.ptr(work), work.numel(), _lib.stream(), ctypes.byref(handle)) == -3
    assert not handle.value
    # form 3 without weights: an argument error, nothing launched
    op.obs_w = None
    assert lib.mgp_operator_apply(ctypes.byref(op), _lib.ptr(X), 1, _lib.ptr(Y), _lib.ptr(work), work.numel(),
                                  _lib.stream()) == -1
    # the Lanczos tridiagonalisation takes form 3 (SPD): finite coefficients
    op = desc.with_(form=3, noise=1e-2, obs_w=w).struct()
    steps = 8
    wb = lib.mgp_lanczos_tridiag_workspace_bytes(ctypes.byref(op), steps)
    assert wb > 0
    lw = torch.empty(wb, dtype=torch.uint8, device=dev)
    alpha, beta = (ctypes.c_float * steps)(), (ctypes.c_float * steps)()
    q0 = torch.randn(n, device=dev)
    _lib.check(lib.mgp_lanczos_tridiag(ctypes.byref(op), _lib.ptr(q0), steps, alpha, beta, None, _lib.ptr(lw), wb,
                                       _lib.stream()), "mgp_lanczos_tridiag")
    a = np.array(alpha[:])
    wn = w.double().cpu().numpy()
    lam_max = np.linalg.eigvalsh(np.diag(wn) + 1e-2 * ref.device_q2(desc).toarray()).max()
    assert np.isfinite(a).all() and (a > 0).all() and (a <= lam_max * 1.0001).all()


def test_form3_lanczos_block_matches_single(mgp, golden, dev):
    """mgp_lanczos_tridiag_block (declared form-3 capable in the header) on form 3: every column's alpha / beta equal the
    single-vector mgp_lanczos_tridiag of that column, and the Ritz values lie inside the spectrum of diag(w) + s Q2."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    g = golden("dumbbell_k10_loop")
    desc = _desc(mgp, g, dev, "randomwalk", 2)
    n, s, P, steps = desc.n, 1e-2, 4, 8
    w = _weights(n, dev, 6)
    op = desc.with_(form=3, noise=s, obs_w=w).struct()
    Q0 = torch.randn(n, P, device=dev)
    wb = lib.mgp_lanczos_tridiag_block_workspace_bytes(ctypes.byref(op), P, steps)
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    ab, bb = (ctypes.c_float * (steps * P))(), (ctypes.c_float * (steps * P))()
    _lib.check(lib.mgp_lanczos_tridiag_block(ctypes.byref(op), _lib.ptr(Q0), P, steps, ab, bb, _lib.ptr(work), wb,
                                             _lib.stream()), "mgp_lanczos_tridiag_block")
    ab, bb = np.array(ab[:]).reshape(steps, P), np.array(bb[:]).reshape(steps, P)
    ev = np.linalg.eigvalsh(np.diag(w.double().cpu().numpy()) + s * ref.device_q2(desc).toarray())
    ws = lib.mgp_lanczos_tridiag_workspace_bytes(ctypes.byref(op), steps)
    w1 = torch.empty(ws, dtype=torch.uint8, device=dev)
    for j in range(P):
        a1, b1 = (ctypes.c_float * steps)(), (ctypes.c_float * steps)()
        q0 = Q0[:, j].contiguous()
        _lib.check(lib.mgp_lanczos_tridiag(ctypes.byref(op), _lib.ptr(q0), steps, a1, b1, None, _lib.ptr(w1), ws,
                                           _lib.stream()), "mgp_lanczos_tridiag")
        assert np.allclose(ab[:, j], np.array(a1[:]), rtol=1e-4, atol=1e-6 * ev.max()), j
        assert np.allclose(bb[:steps - 1, j], np.array(b1[:steps - 1]), rtol=1e-3, atol=1e-6 * ev.max()), j
        Tm = np.diag(ab[:, j]) + np.diag(bb[:steps - 1, j], 1) + np.diag(bb[:steps - 1, j], -1)
        rv = np.linalg.eigvalsh(Tm)
        assert rv.min() >= ev.min() * (1 - 1e-3) - 1e-6 * ev.max() and rv.max() <= ev.max() * (1 + 1e-4), j


# ------------------------------------------------------------------------------------------------ 6: samples vs float64
_DENSE = {}


def _dense(g, norm, nu, scale):
    key = (id(g), norm, nu)
    if key not in _DENSE:
        lo = ref.oracle(g, norm)
        kappa = float(g["kappa"])
        n = lo.n
        tau = 2.0 * nu / kappa ** 2
        A = tau * np.eye(n) + lo.dense_symmetric()
        P = np.sqrt(lo.degree) if norm == "randomwalk" else np.ones(n)
        from oracle.precision import dense_matern_precision
        Q2 = scale * dense_matern_precision(lo.dense(), nu, kappa, lo.degree if norm == "randomwalk" else None)
        r, c = lo.idx[0], lo.idx[1]
        E = edge_factor(n, r, c, lo.triu, np.sqrt(lo.degree)) if nu % 2 else None
        _DENSE.clear()
        _DENSE[key] = dict(n=n, tau=tau, A=A, P=P, Q2=Q2, r=r, c=c, E=E)
    return _DENSE[key]


def _z_ref(d, nu, scale, seed, S):
    w = node_noise(d["n"], 0, seed, 0, S)
    if nu % 2:
        noise, k = math.sqrt(d["tau"]) * w + d["E"] @ edge_noise(d["r"], d["c"], seed, 0, S), (nu - 1) // 2
    else:
        noise, k = w, nu // 2
    return math.sqrt(scale) * d["P"][:, None] * (np.linalg.matrix_power(d["A"], k) @ noise)


def _colerr(x, want):
    return float((np.abs(x - want).max(axis=0) / np.abs(want).max(axis=0)).max())


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_observed_samples_vs_dense_fp64(mgp, golden, dev, norm, nu):
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k10_loop")
    scale, s, S, seed = 0.8, 1e-2, 5, 777
    desc = _desc(mgp, g, dev, norm, nu, scale)
    d = _dense(g, norm, nu, scale)
    n = d["n"]
    z = _z_ref(d, nu, scale, seed, S)
    w2, w3 = node_noise(n, 2, seed, 0, S), node_noise(n, 3, seed, 0, S)
    y = g["train_y"].astype(np.float64)
    rng = np.random.default_rng(nu)
    for frac in (0.1, 0.5):
        obs = rng.random(n) < frac
        y_nan = np.where(obs, y, np.nan).astype(np.float32)
        for per_node in (False, True):
            var = s * rng.uniform(0.5, 2.0, n) if per_node else np.full(n, s)
            noise = T(var.astype(np.float32), dev) if per_node else s
            var32 = var.astype(np.float32).astype(np.float64) if per_node else var
            ob = T(obs, dev)
            kw = dict(tol=1e-6, refine=3, observed=ob)
            mean = sampling.posterior_mean(desc, T(y_nan, dev), noise, **kw).double().cpu().numpy()
            assert _colerr(mean[:, None], ref.mean(d["Q2"], y, var32, obs)[:, None]) < 1e-4
            x = sampling.posterior_samples(desc, T(y_nan, dev), noise, S, seed, **kw).double().cpu().numpy().T
            want = ref.samples(d["Q2"], y, var32, obs, z, w2)
            assert np.isfinite(x).all()
            assert _colerr(x, want) < 1e-4, (frac, per_node, _colerr(x, want))
            xn = sampling.posterior_samples(desc, T(y_nan, dev), noise, S, seed, noisy=True, **kw).double().cpu().numpy().T
            assert _colerr(xn, want + np.sqrt(var32)[:, None] * w3) < 1e-4
            rhs = sampling.posterior_rhs(desc, T(y_nan, dev), noise, S, seed, observed=ob).double().cpu().numpy()
            assert _colerr(rhs, ref.perturbed_rhs(y, var32, obs, z, w2)) < 1e-5


# ------------------------------------------------------------------------------------------------ 7: statistics
def test_observed_sample_statistics(mgp, golden, dev):
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k10_loop")
    scale, S, nu, norm = 1.3, 2048, 2, "randomwalk"
    desc = _desc(mgp, g, dev, norm, nu, scale)
    d = _dense(g, norm, nu, scale)
    n = d["n"]
    rng = np.random.default_rng(21)
    obs = rng.random(n) < 0.3
    var = (5e-2 * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    y = T(g["train_y"], dev)
    x = sampling.posterior_samples(desc, y, T(var, dev), S, 19, observed=T(obs, dev)).double().cpu().numpy()
    mean = sampling.posterior_mean(desc, y, T(var, dev), observed=T(obs, dev)).double().cpu().numpy()
    cov = np.linalg.inv(d["Q2"] + np.diag(np.where(obs, 1.0 / var.astype(np.float64), 0.0)))
    V = rng.standard_normal((n, 8))
    dev_ = (x - mean[None, :]) @ V
    want = np.einsum("ip,ij,jp->p", V, cov, V)
    got = (dev_ ** 2).mean(0)
    assert (np.abs(got / want - 1.0) < 6.0 * math.sqrt(2.0 / S)).all(), got / want
    assert (np.abs(dev_.mean(0)) < 6.0 * np.sqrt(want / S)).all()


# ------------------------------------------------------------------------------------------------ 8: today's sampler
def test_agreement_with_form2_sampler(mgp, golden, dev):
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k50_noloop")
    desc = _desc(mgp, g, dev, "symmetric", 2)
    n, s, seed = desc.n, 2e-2, 31
    y = T(g["train_y"], dev)
    kw = dict(tol=1e-6, refine=3)
    const = torch.full((n,), s, device=dev)
    m2 = sampling.posterior_mean(desc, y, s, **kw).double().cpu().numpy()
    m3 = sampling.posterior_mean(desc, y, const, **kw).double().cpu().numpy()
    assert _colerr(m3[:, None], m2[:, None]) < 1e-5
    x2 = sampling.posterior_samples(desc, y, s, 6, seed, **kw).double().cpu().numpy()
    x3 = sampling.posterior_samples(desc, y, const, 6, seed, **kw).double().cpu().numpy()
    assert _colerr(x3.T, x2.T) < 1e-5
    # observed=None and an all-True mask with a float noise: today's path, bit for bit
    allobs = torch.ones(n, dtype=torch.bool, device=dev)
    a = sampling.posterior_samples(desc, y, s, 6, seed)
    assert torch.equal(a, sampling.posterior_samples(desc, y, s, 6, seed, observed=None))
    assert torch.equal(a, sampling.posterior_samples(desc, y, s, 6, seed, observed=allobs))
    assert torch.equal(sampling.posterior_mean(desc, y, s), sampling.posterior_mean(desc, y, s, observed=allobs))


def test_plan_cache_across_masks_on_relabelled_graph(mgp, dev):
    """posterior_mean with a sequence of masks on a graph whose solves run on the relabelled matrix (the plan keeps only the
    permuted weights): the relabelled data's cache of permuted vectors is emptied between calls, so that nothing but the plan
    could keep a caller's weight tensor -- whose address is the plan's value key -- alive.  Every mean matches its own
    float64 reference, and every cached form-3 plan holds the tensors its value key names."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from manifold_gp_amd import sampling, solvers
    desc = _curve_desc(mgp, dev, "randomwalk", 2, n0=6000, shuffle=True)
    rel = desc.data.relabelled()
    assert rel is not None and desc.relabelled()[0] is not None
    n, s = desc.n, 1e-2
    Q2 = ref.device_q2(desc)
    y = torch.randn(n, device=dev)
    yn = y.double().cpu().numpy()
    solvers.clear_plan_cache()
    rng = np.random.default_rng(12)
    try:
        for it in range(4):
            obs = rng.random(n) < (0.3 if it % 2 else 0.6)
            rel._perm_cache.clear()
            m = sampling.posterior_mean(desc, y, s, tol=1e-7, refine=4, observed=T(obs, dev)).double().cpu().numpy()
            A3 = (sp.diags(obs.astype(np.float64)) + s * Q2).tocsc()
            want = spla.spsolve(A3, obs * yn)
            assert np.abs(m - want).max() <= 1e-4 * np.abs(want).max(), it
            for plan in solvers._PLAN_CACHE.values():
                if plan.desc.form == 3:
                    held = [t.data_ptr() for t in plan._keep if t is not None]
                    assert plan._vkey[-1] in held
    finally:
        solvers.clear_plan_cache()


# ------------------------------------------------------------------------------------------------ 9: model API, chunking
def _model(mgp, g, dev, labeled=None):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    x, y = T(g["train_x"], dev), T(g["train_y"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=3, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    return RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev), labeled=labeled).to(dev)


def test_model_observed_api_and_chunking(mgp, golden, dev):
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    model = _model(mgp, g, dev)
    obs = np.random.default_rng(2).random(n) < 0.5
    ob = T(obs, dev)
    mean = model.precision_posterior_mean(tol=1e-6, observed=ob)
    assert mean.shape == (n,) and mean.dtype == torch.float32
    desc = model.precision(noise=False)._descriptor()
    noise = float(model.likelihood.noise.detach().reshape(-1)[0])
    Q2 = ref.device_q2(desc).toarray()
    want = ref.mean(Q2, g["train_y"].astype(np.float64), np.full(n, noise), obs)
    got = mean.double().cpu().numpy()
    assert np.abs(got - want)[~obs].max() / np.abs(want).max() < 1e-4
    out = model.sample_posterior(4, seed=3, observed=ob)
    assert out.shape == (4, n) and torch.isfinite(out).all()
    assert torch.equal(out, model.sample_posterior(4, seed=3, observed=ob))
    # chunks of 256 columns: the first chunk is the same solve; the columns behind it agree to the tolerance
    from manifold_gp_amd import sampling
    y = T(g["train_y"], dev)
    a = sampling.posterior_samples(desc, y, noise, 300, 5, tol=1e-6, refine=2, observed=ob)
    b = sampling.posterior_samples(desc, y, noise, 260, 5, tol=1e-6, refine=2, observed=ob)
    assert torch.equal(a[:256], b[:256])
    assert _colerr(a[256:260].double().cpu().numpy().T, b[256:260].double().cpu().numpy().T) < 1e-4
    semi = _model(mgp, g, dev, labeled=T(np.arange(n) < 100, dev))
    for fn in (lambda: semi.sample_posterior(2, seed=1, observed=ob), lambda: semi.precision_posterior_mean(observed=ob)):
        with pytest.raises(NotImplementedError):
            fn()


# ------------------------------------------------------------------------------------------------ 10: 60k
def test_observed_manifold784_at_size(mgp, dev):
    """60k manifold_784 graph (k = 50, random walk, nu = 2), 10 % observed: the mean against a float64 scipy CG on W + s Q2,
    and every one of S = 16 samples meets tol on the float64 true residual of its perturbed system."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from manifold_gp_amd import sampling
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    n, k, nu, eps, kappa, s, noise, S, seed, tol = 60000, 50, 2, 0.3, 3.0, 1.0, 1e-2, 16, 2026, 1e-5
    x_np, y_np, _ = synth.manifold_784(n)
    x, y = T(x_np, dev), T(y_np, dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=k, laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=eps, lengthscale=kappa)
    model = RiemannGP(x, y, GaussianLikelihood(noise).to(dev), ScaleKernel(kern, s).to(dev)).to(dev)
    obs = np.random.default_rng(10).random(n) < 0.1
    ob = T(obs, dev)
    desc = model.precision(noise=False)._descriptor()
    Q2 = ref.device_q2(desc)
    W = sp.diags(obs.astype(np.float64))
    A3 = (W + noise * Q2).tocsr()
    b = obs * y_np.astype(np.float64)
    try:
        xr, info = spla.cg(A3, b, rtol=1e-11, maxiter=20000)
    except TypeError:
        xr, info = spla.cg(A3, b, tol=1e-11, maxiter=20000)
    assert info == 0
    # (forward error: a refined solve, whose float64 true residual sits at the fp32 floor)
    mean = sampling.posterior_mean(desc, y, noise, tol=1e-7, refine=4, observed=ob).double().cpu().numpy()
    assert np.abs(mean - xr).max() / np.abs(xr).max() < 1e-4
    assert model.precision_posterior_mean(observed=ob).shape == (n,)
    # solved to tol / 2 on the recurrence residual: the float64 true residual of the fp32 solution then meets tol (solved to tol
    # itself, it lands within a few 1e-9 of tol either side: the C1 rule of tests/test_gpu_solver_contract.py allows 2 tol)
    xs = model.sample_posterior(S, seed=seed, tol=tol / 2, observed=ob).double().cpu().numpy().T
    rhs = sampling.posterior_rhs(desc, y, noise, S, seed, observed=ob).double().cpu().numpy()
    rel = np.linalg.norm(rhs - A3 @ xs, axis=0) / np.linalg.norm(rhs, axis=0)
    assert rel.max() <= tol, rel
