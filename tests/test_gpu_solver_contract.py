"""GPU tests: every CG path held to ONE written contract, checked against float64 references built outside the HIP kernels.

R1 -- the system the solver actually solves: a float64 scipy CSR of B = tau I + L_sym from the operator's own fp32
coefficients (laplacian_diag, laplacian_triu on the graph's index pairs, degree_mat for the random-walk pre / post), then
A = form(scale diag(post) B^nu diag(pre)) applied in float64 (_descriptor.py, operator.hip).  Every residual below is
computed here, never with desc.apply or the library's fp64 apply.
R2 -- the converged oracle: oracle.laplacian.LaplacianOracle(float64) + oracle.sparse.SparsePrecision, for forward errors.
Floor -- F_c = 4 eps32 ||A||_2 ||x_c|| / ||b_c|| (||A||_2 from eigsh on R1); every case asserts F <= tol / 4 at the
tolerance it tests, so that no check passes vacuously.

Contract, per column c:
  C1  stop_mode 1, status 1: true_rel_c <= 2 tol + F_c.
  C2  stop_mode 0, status 1: mean(true_rel) <= 2 tol + mean(F) and iters >= min(10, n - 1) (linear_cg's rule).
  C3  `resid` is honest: refine 0: true_rel_c <= 2 resid_c + F_c; refine > 0 (fp64 true residual of the fp64 solution):
      |resid_c - true_rel_c| <= 1e-2 true_rel_c + 1e-9.
  C4  max_iter exit: status 2, iters == max_iter, C3 holds.
  C5  a zero column gives x == 0 exactly and resid 0; mixed into a block it changes neither the other columns'
      iterations nor their C1.
  C6  forward error against R2: ||x - x*|| / ||x*|| <= 2 cond(A) true_rel + 1e-5 (dumbbell: dense cond is cheap).

Past the caps (test_past_caps_*): C1-C5 again on a 300,071-node swiss roll (tests/_past_caps.py), where the SpMM families give a
workgroup two tiles or several passes and leave 2,345 ... 9,378 delta partials: the C = 1 kernels with 16 delta slots, the
complex-shift update past 1024 partials, the tail loop of cg_update_kernel, cg_reduce_kernel past its first trip.  Every case
asserts its partial count and kernel family (mgp_spmm_dot_blocks_csr, mgp_spmm_kernel_choice on the plan's own CSR) and 20
iterations or more; C6 is left out (it needs a dense matrix).  One-off cost: 0.5-0.7 s per operator for R1 and its norm."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


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


def f32(v):
    return float(np.float32(v))


class R1:
    """float64 A = form(scale diag(post) (tau I + L_sym)^nu diag(pre)) from the operator's fp32 coefficients."""

    def __init__(self, lap, desc):
        n = lap.shape[0]
        ei = lap.graph.edge_index.cpu().numpy()
        s = lap.laplacian_triu.double().cpu().numpy()
        S = sp.coo_matrix((s, (ei[0], ei[1])), shape=(n, n)).tocsr()
        L = (sp.diags(lap.laplacian_diag.double().cpu().numpy()) - S - S.T).tocsr()
        self.nu, self.form, self.n = int(desc.nu), int(desc.form), n
        self.tau = 2.0 * self.nu / (f32(desc.kappa) ** 2)
        self.B = (self.tau * sp.eye(n) + L).tocsr()
        self.scale, self.noise = f32(desc.scale), f32(desc.noise)
        assert (desc.pre is None) == (desc.post is None)
        self.d = np.sqrt(lap.degree_mat.double().cpu().numpy())[:, None] if desc.pre is not None else None
        self._norm = None

    def q2(self, V):
        o = V * self.d if self.d is not None else V
        for _ in range(self.nu):
            o = self.B @ o
        if self.d is not None:
            o = o * self.d
        return self.scale * o

    def apply(self, V):
        V = np.asarray(V, np.float64)
        if self.form == 0:
            return self.q2(V)
        if self.form == 2:
            return V + self.noise * self.q2(V)
        q = self.q2(V)                                   # form 1: Q2 (I - s Q2 (I - s Q2)) = Q2 - s Q2^2 + s^2 Q2^3
        q2 = self.q2(q)
        return q - self.noise * q2 + self.noise ** 2 * self.q2(q2)

    @property
    def norm2(self):
        if self._norm is None:
            op = spla.LinearOperator((self.n, self.n), matvec=lambda v: self.apply(v.reshape(-1, 1)).ravel(), dtype=np.float64)
            self._norm = float(spla.eigsh(op, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0])
        return self._norm

    def dense(self):
        return self.apply(np.eye(self.n))


def contract(sys, B, X, tol, stop_mode, status, iters, resid, refine=0, max_iter=None, X64=None, label=""):
    """C1-C5 of the module docstring for one solve; returns (true_rel, F) per column."""
    B = np.asarray(B.cpu() if torch.is_tensor(B) else B, np.float64).reshape(sys.n, -1)
    X = np.asarray(X.cpu() if torch.is_tensor(X) else X, np.float64).reshape(sys.n, -1)
    Xr = X if X64 is None else np.asarray(X64.cpu(), np.float64).reshape(sys.n, -1)
    resid = np.asarray(resid, np.float64).reshape(-1)
    bn = np.linalg.norm(B, axis=0)
    nz = bn > 0
    true_rel = np.zeros(B.shape[1])
    true_rel[nz] = np.linalg.norm(B - sys.apply(Xr), axis=0)[nz] / bn[nz]
    F = np.zeros(B.shape[1])
    F[nz] = 4 * EPS32 * sys.norm2 * np.linalg.norm(X, axis=0)[nz] / bn[nz]
    info = "%s tol %g status %d iters %d true_rel/tol %s resid/tol %s F/tol %s" % (
        label, tol, status, iters, np.round(true_rel / tol, 3), np.round(resid / tol, 3), np.round(F / tol, 3))
    print(info)
    assert F[nz].max() <= tol / 4, "floor too close to tol: " + info          # not vacuous
    # C5: zero columns
    assert np.all(X[:, ~nz] == 0.0) and np.all(resid[~nz] == 0.0), info
    if status == 1 and stop_mode == 1:                                            # C1
        assert np.all(true_rel[nz] <= 2 * tol + F[nz]), "C1: " + info
    if status == 1 and stop_mode == 0:                                            # C2
        assert true_rel.mean() <= 2 * tol + F.mean(), "C2: " + info
        assert iters >= min(10, sys.n - 1), "C2 iters: " + info
    if refine == 0:                                                               # C3
        assert np.all(true_rel[nz] <= 2 * resid[nz] + F[nz]), "C3: " + info
    else:
        assert np.all(np.abs(resid - true_rel) <= 1e-2 * true_rel + 1e-9), "C3 (refined): " + info
    if max_iter is not None:                                                      # C4
        assert status == 2 and iters == max_iter, "C4: " + info
    return true_rel, F


def forward_error(sys, lo_args, desc, X, true_rel, rhs):
    """C6 against R2: the oracle operator (float64 Laplacian from the edges) solved to 1e-13."""
    from oracle.laplacian import LaplacianOracle
    from oracle.sparse import SparsePrecision
    lo = LaplacianOracle(*lo_args, dtype=np.float64)
    P = SparsePrecision(lo, desc.nu, desc.kappa, scale=desc.scale)
    if desc.form == 2:
        A2 = lambda v: P.posterior_system(v, desc.noise)
    else:
        A2 = P.matmul
    X = np.asarray(X.cpu(), np.float64).reshape(sys.n, -1)
    rhs = np.asarray(rhs.cpu(), np.float64).reshape(sys.n, -1)
    ev = np.linalg.eigvalsh(0.5 * (sys.dense() + sys.dense().T))
    cond = ev.max() / ev.min()
    for c in range(X.shape[1]):
        xs = P.solve(rhs[:, c], matvec=A2, tol=1e-13)
        err = np.linalg.norm(X[:, c] - xs) / np.linalg.norm(xs)
        assert err <= 2 * cond * true_rel[c] + 1e-5, ("C6", c, err, cond, true_rel[c])


# ----------------------------------------------------------------------------- fixtures: graphs and right-hand sides
@pytest.fixture(scope="module")
def dumbbell(mgp, golden, dev):
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    out = {"g": g, "n": n, "kappa": float(g["kappa"])}
    for norm in ("symmetric", "randomwalk"):
        out[norm] = mgp.operators.GraphLaplacianOperator(T(g["edge_value"], dev), T(g["edge_index"].astype(np.int64), dev), n,
                                                         torch.tensor([[float(g["eps"])]], device=dev), norm, bool(g["self_loops"]))
        out["lo_" + norm] = (g["edge_value"], g["edge_index"], n, float(g["eps"]), norm, bool(g["self_loops"]))
    out["y"] = T(g["train_y"], dev).view(-1, 1).contiguous()
    out["gauss"] = torch.randn(n, 1, generator=torch.Generator().manual_seed(41)).to(dev)
    return out


@pytest.fixture(scope="module")
def swiss_roll(mgp, dev):
    from tools import synth
    x_np, y_np = synth.swiss_roll(20000, seed=5, order="morton")
    knn = mgp.utils.NearestNeighbors(T(x_np, dev))
    idx, val = knn.graph(16)
    out = {"n": 20000, "y": T(y_np, dev).view(-1, 1).contiguous(),
           "gauss": torch.randn(20000, 1, generator=torch.Generator().manual_seed(42)).to(dev)}
    for norm in ("symmetric", "randomwalk"):
        out[norm] = mgp.operators.GraphLaplacianOperator(val, idx, 20000, torch.tensor([[0.35]], device=dev), norm,
                                                         graph=knn.knn_graph)
    return out


# The 300,071-node swiss roll of tests/_past_caps.py: past every size cap of the solver's kernels (module docstring, "Past the caps").
# Two conditions choose the systems: (a) every solve takes 20 iterations or more -- a near-identity system stops in two or three
# steps and flips the parity buffers once --, (b) the module's rule F <= tol / 4 holds at tol 1e-3 and 1e-4.
# B = tau I + L_sym has its spectrum in [tau, tau + 585] on this graph (the Laplacian scales with 1 / eps^2 = 503), so kappa is
# chosen through tau = 2 nu / kappa^2; kappa = 4, nu = 2 (tau = 0.25) would give cond(A) = 5e6 and break (b).  Checked beforehand
# with a float64 CG on oracle.laplacian.LaplacianOracle over k-d tree neighbours of the same points, Gaussian and one-hot
# right-hand sides:
#   form 0, nu 2.  tau = 73: 28 / 38 iterations (symmetric, tol 1e-3 / 1e-4) and 31 / 44 (random walk), F / tol at 1e-4 up to 0.11;
#   tau = 40: 53 / 71 and 77 / 103, F / tol up to 0.22.  Used: tau = 55 (kappa = 0.2697, cond(A) = 135).  Measured on the GPU:
#   40 / 53 and 58 / 78 iterations, F / tol <= 0.17.
#   form 2, nu 2, symmetric, for the complex-shift solve alone.  tau = 5 (kappa = 0.8944), noise x scale = 1e-2, cond(A) = 2800:
#   COCG 26 iterations at tol 1e-3 with F / tol = 0.07 (measured on the GPU: 41 and 0.11); at 1e-4 F / tol would be about 0.7, so this
#   system runs at 1e-3 only.
BIG_KAPPA, BIG_SCALE = 0.2697, 4e-6          # ||A||_2 ~ 1.6
BIG_CX_KAPPA, BIG_CX_NOISE = 0.8944, 1e-2
BIG_MIN_ITERS = 20


@pytest.fixture(scope="module")
def swiss300k(mgp, dev):
    """Operators on the 300,071-node graphs: generation order (symmetric, randomwalk; the plans iterate on the relabelled matrix) and
    Z-curve order (randomwalk).  The float64 systems R1 and their ||A||_2 are computed once each (`_big`)."""
    import _past_caps
    out = {"n": _past_caps.N, "sys": {}}
    for order, norms in (("random", ("symmetric", "randomwalk")), ("morton", ("randomwalk",))):
        g = _past_caps.swiss300k(mgp, dev, order)
        out[order] = {norm: mgp.operators.GraphLaplacianOperator(g["val"], g["idx"], out["n"], torch.tensor([[g["eps"]]], device=dev),
                                                                 norm, graph=g["graph"]) for norm in norms}
    out["gauss"] = torch.randn(out["n"], 1, generator=torch.Generator().manual_seed(43)).to(dev)
    return out


def _desc(mgp, lap, nu, kappa, dev, form=2, scale=0.7, noise=1e-2):
    Q = mgp.operators.PrecisionMaternOperator(lap, nu, torch.tensor([[kappa]], device=dev))
    d = Q._descriptor()
    return d.with_(scale=scale, form=2, noise=noise) if form == 2 else d.with_(scale=scale) if form == 0 else d


def _block(n, C, dev, seed):
    """One-hot plus Gaussian columns, as `_average_variance` mixes them."""
    gen = torch.Generator().manual_seed(seed)
    B = torch.randn(n, C, generator=gen)
    h = C // 2
    B[:, :h] = 0.0
    B[torch.randint(0, n, (h,), generator=gen), torch.arange(h)] = 1.0
    return B.to(dev).contiguous()


def _plan_solves(desc, rhs, tol, stop_mode=1, refine=0, max_iter=20000, repeats=3, **kw):
    """The same solve `repeats` times on one plan (the second solve captures the graphs): every solve's report."""
    from manifold_gp_amd.solvers import CgPlan
    plan = CgPlan(desc, rhs.shape[1], tol=tol, max_iter=max_iter, stop_mode=stop_mode, check_every=8, refine=refine, **kw)
    recs = []
    try:
        for _ in range(repeats):
            x = plan.solve(rhs).clone()
            x64 = plan.solution64_view().clone() if refine else None
            recs.append((x, plan.iters, plan.status, plan.resid, x64))
        cx = plan.complex_shift
    finally:
        plan.close()
    return recs, cx


def _check_plan(sys, desc, rhs, tol, stop_mode=1, refine=0, max_iter=20000, label="", **kw):
    recs, cx = _plan_solves(desc, rhs, tol, stop_mode, refine, max_iter, **kw)
    out = None
    for k, (x, its, st, res, x64) in enumerate(recs):
        assert st in (1, 2), (label, st)
        out = contract(sys, rhs, x, tol, stop_mode, st, its, res, refine=refine, X64=x64,
                       max_iter=max_iter if max_iter < 100 else None, label="%s solve %d" % (label, k))
        if max_iter >= 100:
            assert st == 1, (label, st)
    return recs, cx, out


# ----------------------------------------------------------------------------- COCG (complex-shift) solve
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("tol", [1e-2, 1e-3])
def test_cocg_contract_dumbbell(mgp, dumbbell, dev, tol, use_graph):
    """Form 2, nu 2, symmetric, C = 1 takes the complex-shift solve: refine 0 and 3, graph replay and eager launches, the
    max_iter exit, b = 0; the same system on CG (mgp_cg_set_complex_shift(0))."""
    from manifold_gp_amd import _lib
    lap = dumbbell["symmetric"]
    desc = _desc(mgp, lap, 2, dumbbell["kappa"], dev)
    sys = R1(lap, desc)
    rhss = [("gauss", dumbbell["gauss"])] + ([("train_y", dumbbell["y"])] if tol >= 1e-2 else [])
    lib = _lib.lib()
    prev = lib.mgp_cg_set_complex_shift(1)
    try:
        for name, rhs in rhss:
            recs, cx, (tr, _) = _check_plan(sys, desc, rhs, tol, use_graph=use_graph, label="cocg %s" % name)
            assert cx
            forward_error(sys, dumbbell["lo_symmetric"], desc, recs[-1][0], tr, rhs)
            _check_plan(sys, desc, rhs, tol, refine=3, repeats=2, use_graph=use_graph, label="cocg refine %s" % name)
            _check_plan(sys, desc, rhs, tol, max_iter=3, repeats=2, use_graph=use_graph, label="cocg capped %s" % name)
        z = torch.zeros_like(dumbbell["y"])
        recs, _ = _plan_solves(desc, z, tol, use_graph=use_graph)
        for x, its, st, res, _ in recs:
            assert st == 1 and its == 0 and float(x.abs().max()) == 0.0 and res == [0.0]
        lib.mgp_cg_set_complex_shift(0)
        for name, rhs in rhss:
            _, cx, _ = _check_plan(sys, desc, rhs, tol, use_graph=use_graph, label="cg-on-A %s" % name)
            assert not cx
    finally:
        lib.mgp_cg_set_complex_shift(prev)


@pytest.mark.parametrize("tol", [1e-2, 1e-3, 1e-4])
def test_cocg_contract_swiss_roll(mgp, swiss_roll, dev, tol):
    lap = swiss_roll["symmetric"]
    desc = _desc(mgp, lap, 2, 1.0, dev, scale=1.0)
    sys = R1(lap, desc)
    for name in ("y", "gauss"):
        _, cx, _ = _check_plan(sys, desc, swiss_roll[name], tol, label="cocg swiss %s" % name)
        assert cx


# ----------------------------------------------------------------------------- real CG at C = 1
C1_CASES = [
    # (label, norm, nu, form, tols)
    ("form2_rw_nu2", "randomwalk", 2, 2, (1e-2, 1e-3)),
    ("form2_sym_nu1", "symmetric", 1, 2, (1e-2, 1e-3, 1e-4)),
    ("form2_sym_nu3", "symmetric", 3, 2, (1e-2,)),
    ("form0_sym_nu1", "symmetric", 1, 0, (1e-2, 1e-3)),
    ("form0_rw_nu2", "randomwalk", 2, 0, (1e-2, 1e-3)),
    ("form1_sym_nu2", "symmetric", 2, 1, (1e-2, 1e-3)),
]


@pytest.mark.parametrize("label,norm,nu,form,tols", C1_CASES, ids=[c[0] for c in C1_CASES])
def test_real_cg_c1_contract(mgp, dumbbell, dev, label, norm, nu, form, tols):
    """The real Chronopoulos-Gear solve at C = 1: forms 0 / 1 / 2, nu 1-3, both normalisations, Jacobi on / off and the
    init-free start on / off (mgp_cg_set_init_free)."""
    from manifold_gp_amd import _lib
    lap = dumbbell[norm]
    if form == 1:
        base = _desc(mgp, lap, nu, dumbbell["kappa"], dev, form=0, scale=0.6)
        lmax = R1(lap, base).norm2
        desc = base.with_(form=1, noise=0.4 / lmax)               # |s Q2| <= 0.4: the training regime of the noise series
    else:
        desc = _desc(mgp, lap, nu, dumbbell["kappa"], dev, form=form)
    sys = R1(lap, desc)
    lib = _lib.lib()
    try:
        for tol in tols:
            for jac in (False, True):
                for init_free in (1, 0):
                    lib.mgp_cg_set_init_free(init_free)
                    recs, cx, (tr, _) = _check_plan(sys, desc, dumbbell["gauss"], tol, jacobi=jac,
                                                    label="%s jacobi %d init_free %d" % (label, jac, init_free))
                    assert not cx
            if form == 2 and tol == tols[-1]:
                forward_error(sys, dumbbell["lo_" + norm], desc, recs[-1][0], tr, dumbbell["gauss"])
        _check_plan(sys, desc, dumbbell["gauss"], tols[-1], max_iter=4, repeats=2, label=label + " capped")
    finally:
        lib.mgp_cg_set_init_free(1)


# ----------------------------------------------------------------------------- multi-column
@pytest.mark.parametrize("stop_mode", [0, 1])
@pytest.mark.parametrize("C", [4, 12, 17, 100])
def test_multicolumn_contract(mgp, dumbbell, dev, C, stop_mode):
    """C in {4, 12, 17, 100}: the element update and the quad update (mgp_cg_set_update_quads), reduce-once above 16
    columns, the matrix-core SpMM at 48 and more; one-hot plus Gaussian columns; a zero column in the block."""
    from manifold_gp_amd import _lib
    lap = dumbbell["randomwalk"]
    desc = _desc(mgp, lap, 2, dumbbell["kappa"], dev)
    sys = R1(lap, desc)
    B = _block(dumbbell["n"], C, dev, seed=C)
    lib = _lib.lib()
    try:
        for quads in ((1, 0) if C % 4 == 0 else (1,)):
            lib.mgp_cg_set_update_quads(quads)
            for tol in (1e-2, 1e-3):
                recs, _, _ = _check_plan(sys, desc, B, tol, stop_mode=stop_mode, repeats=2,
                                         label="C=%d stop %d quads %d" % (C, stop_mode, quads))
                if stop_mode == 1:
                    # C5: a zero column in place of the last one: same iterations, the other columns unchanged
                    Bz = B.clone()
                    Bz[:, -1] = 0.0
                    Bd = B.clone()
                    Bd[:, -1] = B[:, 0]                                  # a copy of column 0 stops with column 0
                    rz, _, _ = _check_plan(sys, desc, Bz, tol, repeats=1, label="C=%d zero column" % C)
                    rd, _ = _plan_solves(desc, Bd, tol, repeats=1)
                    assert rz[0][1] == rd[0][1], (rz[0][1], rd[0][1])
                    xz, xd = rz[0][0][:, :-1], rd[0][0][:, :-1]
                    assert float((xz - xd).abs().max()) <= 1e-6 * float(xd.abs().max())
    finally:
        lib.mgp_cg_set_update_quads(1)


# ----------------------------------------------------------------------------- decide-in-update
@pytest.mark.parametrize("graph", ["dumbbell", "swiss_roll"])
def test_decide_in_update_contract(mgp, request, dev, graph):
    from manifold_gp_amd import _lib
    G = request.getfixturevalue(graph)
    lap = G["randomwalk"]
    desc = _desc(mgp, lap, 2, 1.5 if graph == "swiss_roll" else G["kappa"], dev)
    sys = R1(lap, desc)
    lib = _lib.lib()
    prev = lib.mgp_cg_set_decide_in_update(1)
    try:
        for mode in (1, 0):
            lib.mgp_cg_set_decide_in_update(mode)
            for tol in (1e-2, 1e-3):
                for name in ("y", "gauss"):
                    if graph == "dumbbell" and name == "y" and tol < 1e-2:
                        continue                                 # F(train_y) ~ 3e-4 on the dumbbell: above tol / 4
                    _check_plan(sys, desc, G[name], tol, label="decide %d %s %s" % (mode, graph, name))
            # (the swiss roll's system is near the identity, cond ~1.1: two steps and tol 1e-4 keep it unconverged)
            capped = (1e-3, 5) if graph == "dumbbell" else (1e-4, 2)
            _check_plan(sys, desc, G["gauss"], capped[0], max_iter=capped[1], repeats=2, label="decide %d capped" % mode)
    finally:
        lib.mgp_cg_set_decide_in_update(prev)


# ----------------------------------------------------------------------------- solve_repeated and the factorised cg_solve
@pytest.mark.parametrize("nu", [2, 3])
@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
def test_factorised_solve_contract(mgp, dumbbell, dev, norm, nu):
    """cg_solve's factorised path (form 0, nu >= 2): the `res` it returns is the true relative residual of the whole
    system (C3), and C1 holds; solve_repeated equals nu plan solves in a row, each of which keeps the contract on B."""
    from manifold_gp_amd import solvers
    from manifold_gp_amd.solvers import CgPlan
    lap = dumbbell[norm]
    desc = _desc(mgp, lap, nu, dumbbell["kappa"], dev, form=0)
    sys = R1(lap, desc)
    B = _block(dumbbell["n"], 6, dev, seed=nu)[:, 3:].contiguous()      # Gaussian columns
    for tol in ((1e-2, 1e-3) if nu == 2 else (1e-2,)):
        X, its, res = solvers.cg_solve(desc, B, tol=tol, stop_mode=1, max_iter=20000)
        contract(sys, B, X, tol, 1, 1, its, res, label="factorised %s nu %d" % (norm, nu))
    # solve_repeated on B = tau I + L_sym (the factor the factorised path iterates on)
    import math
    dB = desc.with_(nu=1, kappa=desc.kappa / math.sqrt(nu), scale=1.0, pre=None, post=None)
    sysB = R1(lap, dB)
    plan = CgPlan(dB, B.shape[1], tol=1e-3, max_iter=20000, stop_mode=1)
    try:
        Xr, its, st = plan.solve_repeated(B, nu)
        cur = B
        for k in range(nu):
            nxt = plan.solve(cur).clone()
            contract(sysB, cur, nxt, 1e-3, 1, plan.status, plan.iters, plan.resid, label="factor %d of %d" % (k + 1, nu))
            cur = nxt
        assert st == 1 and torch.equal(Xr, cur)
    finally:
        plan.close()


# ----------------------------------------------------------------------------- partitioned solvers
def _padded(mgp, dumbbell, dev, norm, nu, form, world):
    from manifold_gp_amd.graph import LaplacianData
    from manifold_gp_amd.parallel import RowPartition, pad_graph
    g = dumbbell["g"]
    lap = dumbbell[norm]
    desc = _desc(mgp, lap, nu, dumbbell["kappa"], dev, form=form)
    part = RowPartition(desc.n, world)
    gp = pad_graph(lap.graph, part.n_pad)
    data = LaplacianData(gp, float(g["eps"]), bool(g["self_loops"]))
    sq = data.dsqrt if norm == "randomwalk" else None
    return lap, desc, desc.with_(data=data, pre=sq, post=sq), part


@pytest.mark.parametrize("recurrence", ["pipelined", "chronopoulos-gear"])
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_pcg_contract(mgp, dumbbell, dev, world, recurrence):
    """virtual_pcg_solve at world 2 and 3 (C1 on the assembled solution), PcgPlan at world 1 with refine 0 and 3 (C1, C3),
    both recurrences.  The pipelined recurrence's residual drifts from the true one on the symmetric system (pcg.hip,
    "Attainable accuracy": at tol 1e-3 it stops with a true residual of 4.6-5.5 tol, F = 0.03 tol); its documented guard is
    refinement, so there it is held to C1 at tol 1e-3 through refine 3 and at refine 0 only at 1e-2."""
    from manifold_gp_amd.parallel import PcgPlan, virtual_pcg_solve
    n = dumbbell["n"]
    for norm, nu, form in (("randomwalk", 2, 2), ("symmetric", 2, 2)):
        lap, desc, dd, part = _padded(mgp, dumbbell, dev, norm, nu, form, world)
        sys = R1(lap, desc)
        rhs = dumbbell["gauss"]
        drifts = recurrence == "pipelined" and norm == "symmetric"
        for tol in ((1e-2,) if drifts else (1e-2, 1e-3)):
            x, its, status, _ = virtual_pcg_solve(dd, part, part.pad(rhs.view(-1)), tol=tol, max_iter=20000, stop_mode=1,
                                                  recurrence=recurrence)
            assert status == 1 and float(x[n:].abs().max()) == 0.0
            tr, F = contract(sys, rhs, x[:n], tol, 1, status, its, [1.0], label="virtual pcg world %d %s" % (world, norm))
        _, _, d1, p1 = _padded(mgp, dumbbell, dev, norm, nu, form, 1)
        for refine in ((3,) if drifts else (0, 3)):
            plan = PcgPlan(d1, p1, 0, tol=1e-3, max_iter=20000, stop_mode=1, refine=refine, recurrence=recurrence)
            try:
                x = plan.solve(p1.pad(rhs.view(-1))).clone()[:n]
                # (a refined PCG solve evaluates its true residual in fp32: `resid` is held to the refine-0 form of C3)
                contract(sys, rhs, x, 1e-3, 1, plan.status, plan.iters, [plan.resid], label="PcgPlan refine %d %s" % (refine, norm))
                assert plan.status == 1
            finally:
                plan.close()


def test_distributed_plan_world1_contract(mgp, dumbbell, dev):
    from manifold_gp_amd.parallel import DistCgPlan, init_comm
    n = dumbbell["n"]
    lap, desc, dd, part = _padded(mgp, dumbbell, dev, "randomwalk", 2, 2, 1)
    sys = R1(lap, desc)
    comm = init_comm(0, 1)
    for tol in (1e-2, 1e-3):
        plan = DistCgPlan(dd, part, 0, comm, C=1, tol=tol, stop_mode=1, max_iter=3000)
        try:
            x = plan.solve(part.pad(dumbbell["gauss"]).contiguous()).clone()
            contract(sys, dumbbell["gauss"], x[:n], tol, 1, plan.status, plan.iters, plan.resid, label="DistCgPlan world 1")
            assert plan.status == 1
        finally:
            plan.close()


# ----------------------------------------------------------------------------- past the caps (n = 300,071)
def _big(mgp, G, dev, order, norm, cx=False):
    """(lap, desc, R1) of one 300k operator; R1 and its norm2 (eigsh) once per operator."""
    import time
    key = (order, norm, cx)
    if key not in G["sys"]:
        lap = G[order][norm]
        if cx:
            desc = _desc(mgp, lap, 2, BIG_CX_KAPPA, dev, form=2, scale=1.0, noise=BIG_CX_NOISE)
        else:
            desc = _desc(mgp, lap, 2, BIG_KAPPA, dev, form=0, scale=BIG_SCALE)
        t0 = time.time()
        sys = R1(lap, desc)
        print("R1 %s: ||A||_2 = %.4g (%.1f s)" % (key, sys.norm2, time.time() - t0))
        G["sys"][key] = (lap, desc, sys)
    return G["sys"][key]


def _plan_geometry(desc, C):
    """What a CgPlan of this descriptor and width multiplies with, read off a plan's own CSR while that plan is open (the geometry
    depends on the descriptor, the width and the lab switches, not on tol / max_iter: the plans that _check_plan solves with bind
    the same struct).  dict: nbs = dot partials of the C-column SpMM, family, nbs4 / family4 = the same for the four-column product
    of the complex-shift solve, tile_rows, relabelled = the plan iterates on P A P^T."""
    import ctypes
    from manifold_gp_amd import _lib
    from manifold_gp_amd.solvers import CgPlan
    lib = _lib.lib()
    plan = CgPlan(desc, C, tol=1e-3, max_iter=10, stop_mode=1)
    try:
        L = ctypes.byref(plan.op.L)
        return dict(nbs=lib.mgp_spmm_dot_blocks_csr(L, C), family=lib.mgp_spmm_kernel_choice(L, C, 1, 0),
                    nbs4=lib.mgp_spmm_dot_blocks_csr(L, 4), family4=lib.mgp_spmm_kernel_choice(L, 4, 1, 0),
                    tile_rows=int(plan.op.L.tile_rows), relabelled=plan._rg is not None)
    finally:
        plan.close()


def _big_check(sys, desc, rhs, tol, label, **kw):
    """_check_plan with two solves (the first runs eager launches; the second captures the graphs and runs as their replay); every
    uncapped solve takes BIG_MIN_ITERS steps or more, so that the parity buffers flip many times."""
    recs, cx, out = _check_plan(sys, desc, rhs, tol, repeats=2, label=label, **kw)
    if kw.get("max_iter", 20000) >= 100:
        for _, its, _, _, _ in recs:
            assert its >= BIG_MIN_ITERS, (label, its)
    return recs, cx, out


@pytest.mark.parametrize("decide", [1, 0])
@pytest.mark.parametrize("norm", ["randomwalk", "symmetric"])
def test_past_caps_real_cg_c1(mgp, swiss300k, dev, norm, decide):
    """Real CG at C = 1 with 2,345 delta partials (more than 4 x 256): cg_update_c1_kernel<*, 16> and cg_decide_c1_kernel with 16
    delta slots; random walk (pre / post) and symmetric (the init-free start; complex shift switched off, which form 0 would not
    take anyway); the stopping decision inside the update and as launches of its own.
    Measured: 58 / 78 iterations (random walk, tol 1e-3 / 1e-4) and 40 / 53 (symmetric), the same with either decision form and on
    the graph replay; true_rel <= 0.95 tol; F <= 0.15 tol."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    lap, desc, sys = _big(mgp, swiss300k, dev, "random", norm)
    prev_cx, prev_dec = lib.mgp_cg_set_complex_shift(0), lib.mgp_cg_set_decide_in_update(decide)
    try:
        geo = _plan_geometry(desc, 1)
        assert geo["family"] == 1 and geo["nbs"] > 1024 and geo["relabelled"], geo        # tile SpMV, two tiles per workgroup
        assert geo["nbs"] < -(-swiss300k["n"] // geo["tile_rows"]), geo
        for tol in (1e-3, 1e-4):
            _, cx, _ = _big_check(sys, desc, swiss300k["gauss"], tol, "300k C=1 %s decide %d" % (norm, decide))
            assert not cx
    finally:
        lib.mgp_cg_set_complex_shift(prev_cx)
        lib.mgp_cg_set_decide_in_update(prev_dec)


def test_past_caps_complex_shift(mgp, swiss300k, dev):
    """The complex-shift solve (form 2, nu 2, symmetric) with 2,345 four-column partials per product: cx_update_kernel past 1024.
    Measured: 41 iterations at tol 1e-3, true_rel 0.66 tol, F 0.11 tol."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    lap, desc, sys = _big(mgp, swiss300k, dev, "random", "symmetric", cx=True)
    prev = lib.mgp_cg_set_complex_shift(1)
    try:
        geo = _plan_geometry(desc, 1)
        assert geo["family4"] == 2 and geo["nbs4"] > 1024, geo
        _, cx, _ = _big_check(sys, desc, swiss300k["gauss"], 1e-3, "300k complex shift")
        assert cx
    finally:
        lib.mgp_cg_set_complex_shift(prev)


@pytest.mark.parametrize("C,stop_mode", [(5, 1), (8, 1), (9, 1), (12, 1), (16, 1), (12, 0)])
def test_past_caps_multicolumn_tail_loop(mgp, swiss300k, dev, C, stop_mode):
    """C = 5 ... 16: the element update (cg_update_kernel), every workgroup of which sums all 2,345 delta partials -- more than the
    2 x 32 x TS its first round trip holds (2048 for 5 <= C <= 8, 1024 for 9 <= C <= 16), so the tail loop runs: one further batch
    at C = 5 and 8, three at C = 9 ... 16, the last one partly masked.  C = 12 also carries a zero column and a duplicate column
    (C5 of the contract).
    Measured: 58 / 78 iterations at every width (stop_mode 0 at C = 12: 52 / 72), true_rel <= 1.0 tol per column, F <= 0.17 tol; the
    zero-column and duplicate-column solves take the same 58 steps."""
    lap, desc, sys = _big(mgp, swiss300k, dev, "random", "randomwalk")
    n = swiss300k["n"]
    geo = _plan_geometry(desc, C)
    nbs, family = geo["nbs"], geo["family"]
    TC = 1
    while TC < C:
        TC <<= 1
    assert nbs > 2 * 32 * (256 // TC), (C, nbs)
    assert family == (2 if C % 4 == 0 else 0), (C, family)
    B = _block(n, C, dev, seed=300 + C)
    for tol in (1e-3, 1e-4):
        _big_check(sys, desc, B, tol, "300k C=%d stop %d" % (C, stop_mode), stop_mode=stop_mode)
    if C == 12 and stop_mode == 1:
        tol = 1e-3
        Bz = B.clone()
        Bz[:, -1] = 0.0
        Bd = B.clone()
        Bd[:, -1] = B[:, 0]
        rz, _, _ = _check_plan(sys, desc, Bz, tol, repeats=1, label="300k C=12 zero column")
        rd, _ = _plan_solves(desc, Bd, tol, repeats=1)
        assert rz[0][1] == rd[0][1] and rz[0][1] >= BIG_MIN_ITERS, (rz[0][1], rd[0][1])
        xz, xd = rz[0][0][:, :-1], rd[0][0][:, :-1]
        assert float((xz - xd).abs().max()) <= 1e-6 * float(xd.abs().max())


def test_past_caps_c17_reduce_once(mgp, swiss300k, dev):
    """C = 17: cg_reduce_kernel over 3,126 delta partials (four trips of 1024) and 2 x nbv gamma / rr partials, the element
    update behind it; the gather SpMM with a three-pass row range (96 rows per workgroup).
    Measured: 58 iterations, true_rel <= 1.0 tol."""
    lap, desc, sys = _big(mgp, swiss300k, dev, "random", "randomwalk")
    n = swiss300k["n"]
    geo = _plan_geometry(desc, 17)
    nbs, family = geo["nbs"], geo["family"]
    assert family == 0 and nbs == -(-n // 96) and nbs > 1024 and nbs < -(-n // 32), (family, nbs)
    _big_check(sys, desc, _block(n, 17, dev, seed=317), 1e-3, "300k C=17")


@pytest.mark.parametrize("quads", [1, 0])
@pytest.mark.parametrize("order", ["random", "morton"])
def test_past_caps_c100(mgp, swiss300k, dev, order, quads):
    """C = 100: cg_reduce_kernel past its first trip on every array (about 2,000 update workgroups; 4,096 dictionary partials on the
    generation-order graph, where the matrix-core image is switched off so that rule 4 of spmm_plan decides through big_x; 9,378
    matrix-core partials on the Z-curve graph), the quad update and the element update (mgp_cg_set_update_quads).
    Measured: 58 iterations in all four cases, true_rel <= 1.0 tol; about 2 s a case, most of it the float64 residual on the host."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    lap, desc, sys = _big(mgp, swiss300k, dev, order, "randomwalk")
    n = swiss300k["n"]
    prev_mt = lib.mgp_spmm_set_mt_mode(0 if order == "random" else 1)
    lib.mgp_cg_set_update_quads(quads)
    try:
        geo = _plan_geometry(desc, 100)
        nbs, family = geo["nbs"], geo["family"]
        if order == "random":
            assert family == 5 and nbs == 4096, (family, nbs)
        else:
            assert family == 3 and nbs > 4096, (family, nbs)
        _big_check(sys, desc, _block(n, 100, dev, seed=400), 1e-3, "300k C=100 %s quads %d" % (order, quads))
    finally:
        lib.mgp_spmm_set_mt_mode(prev_mt)
        lib.mgp_cg_set_update_quads(1)


@pytest.mark.parametrize("C", [12, 1])
def test_past_caps_max_iter_exit(mgp, swiss300k, dev, C):
    """C4 on the tail-loop paths: five steps, status 2, and a `resid` that is honest about the unconverged solution."""
    lap, desc, sys = _big(mgp, swiss300k, dev, "random", "randomwalk")
    assert _plan_geometry(desc, C)["nbs"] > 1024
    rhs = swiss300k["gauss"] if C == 1 else _block(swiss300k["n"], C, dev, seed=300 + C)
    _big_check(sys, desc, rhs, 1e-4, "300k C=%d capped" % C, max_iter=5)
