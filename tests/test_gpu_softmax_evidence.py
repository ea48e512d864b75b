"""The Laplace evidence of the softmax fit on the MI355X (mgp_softmax_root_apply and mgp_softmax_curvature in csrc/laplace.hip, the
softmax family of manifold_gp_amd/evidence.py): the two kernels against float64 on the same float32 inputs, logdet B by both
methods, the evidence and its hyper-parameter gradient against the dense float64 restatement (tests/_softmax_evidence_ref.py),
the training loop against its float64 run, and the model method."""
import warnings

import numpy as np
import pytest
import torch

import _evidence_ref as eref
import _observed_ref as obref
import _softmax_evidence_ref as sev
import _softmax_ref as sref
from test_gpu_evidence import _rel_residual, check_theta
from test_gpu_variance import T, _desc

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 257, 4099]
CLASSES = [2, 3, 7, 33, 64]
SAMPLES = [1, 5, 16]
C3 = sev.C_FIT
# logdet B by the dense path against the dense float64 value at the device's mode, |difference| / logdet B: 4 x the worst value
# measured on the MI355X (docs/kernels/evidence.md, "The softmax family": 1.03e-8 and 2.09e-9 on the two fixtures at C = 3, 8.93e-8
# on the 300-node graph at C = 64), never looser than 1e-3
DENSE_MEASURED = 8.93e-8
DENSE_BAR = min(4 * DENSE_MEASURED, 1e-3)
# the Lanczos path against the float64 quadrature on the same probes (16 probes, 12 steps): value, |difference| / logdet B;
# standard error, |difference| / se: 4 x the worst of the two cases measured (1.93e-8 and 2.06e-7 at C = 3, 4.05e-8 and 6.73e-8 at
# C = 64), never looser than 1e-3
SLQ_MEASURED, SLQ_SE_MEASURED = 4.05e-8, 2.06e-7
SLQ_BAR, SLQ_SE_BAR = min(4 * SLQ_MEASURED, 1e-3), min(4 * SLQ_SE_MEASURED, 1e-3)


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


# ------------------------------------------------------------------------------------------------ 1: the two kernels
def _pi(n, C, rng):
    """softmax rows at 70 % of the nodes (row 0 always), rows of zeros elsewhere; the last observed row holds one pi at 1 - 2^-24
    and the rest of the mass in one other class"""
    obs = rng.random(n) < 0.7
    obs[0] = True
    pi = np.where(obs[:, None], sref.softmax(rng.standard_normal((n, C)) * 2.0), 0.0).astype(np.float32)
    last = np.flatnonzero(obs)[-1]
    pi[last] = 0.0
    pi[last, C - 1], pi[last, 0] = np.float32(1.0 - 2.0 ** -24), np.float32(2.0 ** -24)
    return pi, obs


def _within(got, want, scale):
    """1 ulp of the once-rounded reference, or 2^-40 of the row's term scale where the result cancels below that"""
    w32 = want.astype(np.float32)
    with np.errstate(over="ignore"):
        near = np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)
    return near | (np.abs(got.astype(np.float64) - want) <= 2.0 ** -40 * scale)


def _pad(a, dev):
    """the array on the device one float off a 16-byte boundary"""
    t = T(np.concatenate([a.reshape(-1)[:1], a.reshape(-1)]), dev)[1:].view(a.shape)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_root_apply_is_the_once_rounded_float64_product(dev, mgp, n, C):
    """R V, V + R^T X and R^T X for S in {1, 5, 16} wherever C S <= 256, in both layouts, against float64 on the same float32 inputs
    rounded once: 1 ulp, or 2^-40 of the row's term scale.  30 % of the rows unobserved with NaN in V and X there (exactly 0
    forward, exactly V transposed), a row with one pi at 1 - 2^-24, pointers one float off 16-byte alignment, out = V and out = X,
    second calls bitwise equal."""
    from manifold_gp_amd.evidence import softmax_root_apply
    rng = np.random.default_rng(1000 * C + n)
    pi, obs = _pi(n, C, rng)
    pid = T(pi, dev)
    for S in [s for s in SAMPLES if C * s <= 256]:
        for layout in ("cs", "sc"):
            shape = (n, C, S) if layout == "cs" else (n, S, C)
            V, X = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
            Vn, Xn = (np.where(obs[:, None, None], a, np.float32(np.nan)) for a in (V, X))
            label = "n = %d, C = %d, S = %d, %s" % (n, C, S, layout)
            # forward
            want, scale = sev.root_apply(pi, V, layout)
            got = softmax_root_apply(pid, T(Vn, dev), layout=layout)
            g = got.cpu().numpy()
            assert got.dtype == torch.float32 and g.shape == shape and np.isfinite(g).all(), label
            assert _within(g, want, scale).all(), (label, "forward")
            assert not g[~obs].any()
            assert torch.equal(got, softmax_root_apply(pid, T(Vn, dev), layout=layout))                       # bitwise
            assert torch.equal(got, softmax_root_apply(pid, _pad(Vn, dev), out=_pad(np.zeros_like(V), dev), layout=layout))
            alias = T(Vn, dev)
            assert softmax_root_apply(pid, alias, out=alias, layout=layout) is alias and torch.equal(alias, got)
            # transposed, with and without V; V keeps finite values off the observed rows: out = V there bit for bit
            want, scale = sev.root_apply_t(pi, X, V, layout)
            got = softmax_root_apply(pid, T(V, dev), T(Xn, dev), transpose=True, layout=layout)
            g = got.cpu().numpy()
            assert np.isfinite(g).all() and _within(g, want, scale).all(), (label, "transposed")
            assert np.array_equal(g[~obs], V[~obs])
            assert torch.equal(got, softmax_root_apply(pid, _pad(V, dev), _pad(Xn, dev), transpose=True, layout=layout))
            for into in ("V", "X"):
                v, x = T(V, dev), T(Xn, dev)
                out = softmax_root_apply(pid, v, x, transpose=True, out=v if into == "V" else x, layout=layout)
                assert torch.equal(out, got), (label, "out = " + into)
            want, scale = sev.root_apply_t(pi, X, None, layout)
            g = softmax_root_apply(pid, None, T(Xn, dev), transpose=True, layout=layout).cpu().numpy()
            assert _within(g, want, scale).all() and not g[~obs].any(), (label, "R^T X")
    # the row at 1 - 2^-24 is part of every case above; here it is on its own: R v there has the scale 2^-12 |v|
    last = np.flatnonzero(obs)[-1]
    one = np.zeros((n, C, 1), np.float32)
    one[last, 0, 0] = 1.0
    got = softmax_root_apply(pid, T(one, dev)).cpu().numpy()
    want, scale = sev.root_apply(pi, one)
    assert _within(got, want, scale).all() and got[last, 0, 0] > 0 and abs(got[last, 0, 0] / 2.0 ** -12 - 1.0) <= 1e-6


def test_root_apply_refuses_bad_arguments_before_any_launch(dev, mgp):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n, C, S = 64, 3, 4
    pi = torch.full((n, C), 1.0 / 3.0, device=dev)
    V = torch.ones(n, C, S, device=dev)
    out = torch.full((n, C, S), 7.0, device=dev)
    p, st = _lib.ptr, _lib.stream()

    def call(pi_=pi, V_=V, X_=None, n_=n, C_=C, S_=S, cs=S, ss=1, tr=0, out_=out):
        return lib.mgp_softmax_root_apply(p(pi_), p(V_), p(X_), n_, C_, S_, cs, ss, tr, p(out_), st)
    assert call(pi_=None) == -1 and call(V_=None) == -1 and call(out_=None) == -1 and call(X_=V) == -1 and call(tr=1) == -1
    assert call(n_=0) == -1 and call(C_=1) == -1 and call(C_=65) == -1 and call(S_=0) == -1 and call(C_=64, S_=5) == -1
    for cs, ss in ((0, 1), (1, 0), (1, 1), (2, 1), (5, 1), (1, 4), (-4, 1)):
        assert call(cs=cs, ss=ss) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                           # nothing was launched
    assert call() == 0 and call(cs=1, ss=C) == 0 and call(tr=1, X_=V, V_=None) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) <= 1e-6                                                     # R^T 1 = s (1 - sum pi) = 0


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n", SIZES)
def test_curvature_accumulates_the_float64_sums(dev, mgp, n, C):
    """S in {1, 5}: acc and acc2 after one block, and after a second one on top, within 1e-14 of the sum of their absolute terms;
    rows of zeros in pi keep what they held (NaN in delta there); a second run over the same blocks is bitwise equal."""
    from manifold_gp_amd.evidence import softmax_curvature
    rng = np.random.default_rng(77 * C + n)
    pi, obs = _pi(n, C, rng)
    pid = T(pi, dev)
    for S in [s for s in (1, 5) if C * s <= 256]:
        d1, d2 = (rng.standard_normal((n, S, C)).astype(np.float32) * 3.0 for _ in range(2))
        n1, n2 = (T(np.where(obs[:, None, None], a, np.float32(np.nan)), dev) for a in (d1, d2))
        a1, b1, sa1, sb1 = sev.curvature_sums(pi, d1)
        a2, b2, sa2, sb2 = sev.curvature_sums(pi, d2)
        acc, acc2 = softmax_curvature(pid, n1)
        ga, gb = acc.cpu().numpy(), acc2.cpu().numpy()
        assert acc.dtype == torch.float64 and acc.shape == (n, C) and np.isfinite(ga).all() and np.isfinite(gb).all()
        e1 = max((np.abs(ga - a1) / np.where(sa1 > 0, sa1, 1.0)).max(), (np.abs(gb - b1) / np.where(sb1 > 0, sb1, 1.0)).max())
        assert softmax_curvature(pid, n2, acc, acc2)[0] is acc
        ga, gb = acc.cpu().numpy(), acc2.cpu().numpy()
        sa, sb = sa1 + sa2, sb1 + sb2
        e2 = max((np.abs(ga - (a1 + a2)) / np.where(sa > 0, sa, 1.0)).max(), (np.abs(gb - (b1 + b2)) / np.where(sb > 0, sb, 1.0)).max())
        print("curvature n = %d, C = %d, S = %d: one block %.1e, two blocks %.1e of the absolute terms" % (n, C, S, e1, e2))
        assert e1 <= 1e-14 and e2 <= 1e-14
        assert not ga[~obs].any() and not gb[~obs].any()
        again = softmax_curvature(pid, n2, *softmax_curvature(pid, n1))
        assert torch.equal(again[0], acc) and torch.equal(again[1], acc2)                     # bitwise
        keep, keep2 = (torch.full((n, C), v, dtype=torch.float64, device=dev) for v in (7.0, -3.0))
        softmax_curvature(pid, n1, keep, keep2)
        assert bool((keep[T(~obs, dev)] == 7.0).all()) and bool((keep2[T(~obs, dev)] == -3.0).all())      # untouched
        assert torch.equal(keep[T(obs, dev)], (softmax_curvature(pid, n1)[0] + 7.0)[T(obs, dev)])       # one addition to the entry


def test_curvature_refuses_bad_arguments_before_any_launch(dev, mgp):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n, C, S = 64, 3, 4
    pi = torch.full((n, C), 1.0 / 3.0, device=dev)
    delta = torch.ones(n, S, C, device=dev)
    acc, acc2 = (torch.full((n, C), 7.0, dtype=torch.float64, device=dev) for _ in range(2))
    p, st = _lib.ptr, _lib.stream()

    def call(pi_=pi, d_=delta, n_=n, C_=C, S_=S, a_=acc, b_=acc2):
        return lib.mgp_softmax_curvature(p(pi_), p(d_), n_, C_, S_, p(a_), p(b_), st)
    assert call(pi_=None) == -1 and call(d_=None) == -1 and call(a_=None) == -1 and call(b_=None) == -1 and call(b_=acc) == -1
    assert call(n_=0) == -1 and call(C_=1) == -1 and call(C_=65) == -1 and call(S_=0) == -1 and call(C_=64, S_=5) == -1
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all()) and bool((acc2 == 7.0).all())                            # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert float((acc - 7.0).abs().max()) <= 1e-12                                            # delta = 1: d = 0, g = 0


# ------------------------------------------------------------------------------------------------ 2: logdet B and the value
_PROBLEMS = {}


def _problem(mgp, golden, dev, case, norm, nu):
    """One C = 3 problem per (fixture, normalisation, nu), built once: the descriptor scaled to a prior marginal variance of about
    9, the dense float64 matrix the kernels apply, the labels of _softmax_ref.labels, the device's fit and, at the device's mode
    and its float32 pi, the dense evidence."""
    key = (case, norm, nu)
    if key not in _PROBLEMS:
        from manifold_gp_amd.classification import laplace_fit_multiclass
        g = golden(case)
        d1 = _desc(mgp, g, dev, norm, nu, scale=1.0)
        Q1 = obref.device_q2(d1).toarray()
        scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
        desc, Q = d1.with_(scale=scale), scale * Q1
        t, obs, y = sref.labels(g, C3)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*(laplace_fit|CG ).*")
            fit = laplace_fit_multiclass(desc, T(y, dev), C3, T(obs, dev))
        assert fit.converged
        F = fit.mean.double().cpu().numpy()
        solver = sref.Solver(Q, obs)
        _PROBLEMS[key] = dict(g=g, desc=desc, Q=Q, scale=scale, t=t, obs=obs, y=T(y, dev), observed=T(obs, dev), fit=fit, F=F,
                              Pi=fit.pi.double().cpu().numpy(), solver=solver, m=int(obs.sum()), z=sev.log_z(Q, F, t, obs, solver))
    return _PROBLEMS[key]


DENSE_CASES = [("dumbbell_k10_loop", "symmetric", 2), ("dumbbell_k50_noloop", "symmetric", 1)]


@pytest.mark.parametrize("case, norm, nu", DENSE_CASES)
def test_dense_logdet_and_the_evidence_value(mgp, golden, dev, case, norm, nu):
    """C = 3, 10 % observed (m C about 450): "auto" is the dense path; logdet B against the dense float64 value at the device's
    mode within DENSE_BAR, the log-likelihood and the quadratic part within 1e-6 relative.  Measured on the MI355X: 1.03e-8 and
    2.09e-9 (docs/kernels/evidence.md)."""
    from manifold_gp_amd.evidence import logdet_b_softmax
    p = _problem(mgp, golden, dev, case, norm, nu)
    z, fit = p["z"], p["fit"]
    ev = fit.laplace_evidence()
    e_ld, e_ll, e_q = abs(ev.logdet - z["logdet"]) / z["logdet"], abs(ev.log_likelihood - z["log_likelihood"]) / abs(z["log_likelihood"]), \
        abs(ev.quad - z["quad"]) / z["quad"]
    print("%s %s nu = %d: m = %d, logdet B dense %.6f, device %.6f (relative %.2e); log Z %.6f, device %.6f; log-likelihood relative "
          "%.1e, quad relative %.1e" % (case, norm, nu, p["m"], z["logdet"], ev.logdet, e_ld, z["value"], float(ev.value), e_ll, e_q))
    assert p["m"] <= 512 and p["m"] * C3 <= 4096 and ev.method == "dense" and ev.m == p["m"] and ev.se == 0.0 and ev.per_probe is None
    assert e_ld <= DENSE_BAR and e_ll <= 1e-6 and e_q <= 1e-6
    assert ev.value.dtype == torch.float64 and ev.value.shape == () and not ev.value.requires_grad and ev.solves is None
    assert float(ev.value) == ev.log_likelihood - ev.quad - 0.5 * ev.logdet
    assert abs(float(ev.value) - z["value"]) <= 1e-6 * (abs(z["log_likelihood"]) + z["quad"]) + 0.5 * DENSE_BAR * z["logdet"]
    value, se, per = logdet_b_softmax(p["desc"], fit.pi, p["observed"], method="dense")
    assert se == 0.0 and per is None and abs(value - ev.logdet) <= 2 * DENSE_BAR * z["logdet"]


def _check_slq(label, ev_logdet, ev_se, per, per_ref, want, se_ref, dense):
    e_v, e_se = abs(ev_logdet - want) / dense, abs(ev_se - se_ref) / se_ref
    print("slq %s: logdet B dense %.4f, device %.5f +- %.5f, float64 same probes %.5f +- %.5f: |difference| / logdet B = %.2e, se "
          "relative %.2e, worst probe %.2e of logdet B, %.2f standard errors from dense"
          % (label, dense, ev_logdet, ev_se, want, se_ref, e_v, e_se, np.abs(per - per_ref).max() / dense, abs(ev_logdet - dense) / ev_se))
    assert e_v <= SLQ_BAR and e_se <= SLQ_SE_BAR
    assert abs(ev_logdet - dense) <= 5.0 * ev_se


def test_slq_matches_the_float64_quadrature_with_the_same_probes(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, C = 3, 16 given probes and 12 steps against oracle.solvers.slq_logdet_same_probes on the dense B
    at the device's mode: value within SLQ_BAR of logdet B, the standard error within SLQ_SE_BAR relative."""
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    Z = sev.probes(p["obs"], C3, sev.SLQ_PROBES, sev.SLQ_SEED)
    per_ref, want, se_ref = sev.slq_per_probe(p["solver"], p["Pi"], Z, sev.SLQ_STEPS)
    ev = p["fit"].laplace_evidence(method="slq", probes=T(Z.astype(np.float32), dev), steps=sev.SLQ_STEPS, solve_tol=1e-6)
    assert ev.method == "slq" and ev.per_probe.shape == (sev.SLQ_PROBES,) and ev.se == 0.5 * ev.logdet_se and ev.m == p["m"]
    _check_slq("C = 3, m C = %d" % (p["m"] * C3), ev.logdet, ev.logdet_se, ev.per_probe, per_ref, want, se_ref, p["z"]["logdet"])
    default = p["fit"].laplace_evidence(method="slq", num_probes=sev.SLQ_PROBES, steps=sev.SLQ_STEPS, seed=sev.SLQ_SEED)
    assert abs(default.logdet - want) <= SLQ_BAR * p["z"]["logdet"]                            # the default probes are the restatement's


def test_slq_with_64_classes_runs_four_probes_at_a_time(mgp, golden, dev):
    """C = 64 on the graph of the first 300 points of the fixture (k = 10), 20 rows observed with random softmax rows: 256 // 64 = 4
    probes per block of Lanczos vectors, 16 probes in four blocks; against the float64 quadrature on the same probes."""
    from manifold_gp_amd.evidence import _SoftmaxBOperator, logdet_b_softmax
    g = golden("dumbbell_k10_loop")
    n, C, nu = 300, 64, 2
    x = T(g["train_x"][:n], dev)
    knn = mgp.utils.NearestNeighbors(x)
    idx, val = knn.graph(int(g["k"]))
    lap = mgp.operators.GraphLaplacianOperator(val, idx, n, torch.tensor([[float(g["eps"])]], device=dev), "symmetric", graph=knn.knn_graph)
    d1 = mgp.operators.PrecisionMaternOperator(lap, nu, torch.tensor([[float(g["kappa"])]], device=dev))._descriptor().with_(scale=1.0)
    Q1 = obref.device_q2(d1).toarray()
    scale = float(np.float32(np.diag(np.linalg.inv(Q1)).mean() / 9.0))
    desc, Q = d1.with_(scale=scale), scale * Q1
    rng = np.random.default_rng(64)
    obs = np.zeros(n, bool)
    obs[rng.choice(n, 20, replace=False)] = True
    pi = np.where(obs[:, None], sref.softmax(rng.standard_normal((n, C)) * 2.0), 0.0).astype(np.float32)
    Pi, solver = pi.astype(np.float64), sref.Solver(Q, obs)
    dense = sev.logdet_b(solver, Pi)
    Z = sev.probes(obs, C, sev.SLQ_PROBES, sev.SLQ_SEED)
    per_ref, want, se_ref = sev.slq_per_probe(solver, Pi, Z, sev.SLQ_STEPS)
    value, se, per = logdet_b_softmax(desc, T(pi, dev), T(obs, dev), steps=sev.SLQ_STEPS, method="slq", probes=T(Z.astype(np.float32), dev))
    _check_slq("C = 64, m C = %d" % (20 * C), value, se, per, per_ref, want, se_ref, dense)
    op = _SoftmaxBOperator(desc, T(pi, dev), 1e-6, 5000)
    with pytest.raises(ValueError, match="V must be"):
        op.matmul(torch.zeros(n * C, 5, device=dev))                                         # 5 x 64 columns
    auto, se_auto, _ = logdet_b_softmax(desc, T(pi, dev), T(obs, dev))                       # m C = 1280: dense
    print("dense C = 64, m C = %d: logdet B dense %.6f, device %.6f (relative %.2e)" % (20 * C, dense, auto, abs(auto - dense) / dense))
    assert se_auto == 0.0 and abs(auto - dense) <= DENSE_BAR * dense


# ------------------------------------------------------------------------------------------------ 3: the gradient
def _a64(p, X):
    """A X in float64 on the matrix the kernels apply, X [n, C, k]"""
    Pi = p["Pi"][:, :, None]
    return np.einsum("ij,jck->ick", p["Q"], X) + Pi * X - Pi * (Pi * X).sum(1, keepdims=True)


def _rel3(R, B):
    return float((np.sqrt((R * R).sum((0, 1))) / np.sqrt((B * B).sum((0, 1)))).max())


def test_gradient_matches_float64_bilinear_forms(mgp, golden, dev):
    """k10_loop, symmetric, nu = 2, C = 3, 16 given probes, curvature = the dense g at the device's mode: the gradients with respect
    to graph bandwidth, length scale and output scale against the float64 derivatives of the bilinear forms on the device's own u,
    X, Y and mode (oracle/grad_ref.py), within the operator-level bar of test_gpu_gradients.py (2e-4 of the absolute terms); the
    float64 true residuals of X, u and Y <= 2 solve_tol; and the probe term of the output scale's gradient on the device's X and Y
    within 4 of its own standard errors of the dense analytic trace."""
    from oracle.grad_ref import bilinear_grads_f64
    O = mgp.operators
    case, norm, nu, tol = "dumbbell_k10_loop", "symmetric", 2, 1e-6
    p = _problem(mgp, golden, dev, case, norm, nu)
    g, n, Q, F, Pi, solver = p["g"], p["desc"].n, p["Q"], p["F"], p["Pi"], p["solver"]
    theta = [float(np.float32(v)) for v in (float(g["eps"]), float(g["kappa"]), p["scale"])]
    th = [torch.tensor(v, device=dev, requires_grad=True) for v in theta]
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    lap = O.GraphLaplacianOperator(val, idx, n, th[0].view(1, 1), norm, bool(g["self_loops"]))
    op = O.ScaleWrapperOperator(O.PrecisionMaternOperator(lap, nu, th[1]), th[2])
    gd = sev.curvature(solver, Pi)
    P = sev.SLQ_PROBES
    Z = sev.probes(p["obs"], C3, P, 4321)
    ev = p["fit"].laplace_evidence(operator=op, curvature=T(gd, dev), probes=T(Z.astype(np.float32), dev), solve_tol=tol)
    assert ev.value.requires_grad and ev.method == "dense" and set(ev.solves) == {"Z", "u", "X", "Y", "g", "g_se"}
    assert ev.solves["g_se"] is None and all(ev.solves[k].dtype == torch.float64 for k in ("u", "X", "Y"))
    got = [float(x) for x in torch.autograd.grad(ev.value, th)]
    s = {k: v.double().cpu().numpy() for k, v in ev.solves.items() if torch.is_tensor(v)}
    u, X, Y = s["u"], s["X"], s["Y"]
    assert u.shape == (n, C3) and X.shape == (n, C3, P) and Y.shape == (n, C3, P) and np.array_equal(s["Z"], Z)
    V = np.concatenate([F, Y.reshape(n, C3 * P)], 1)
    W = np.concatenate([0.5 * (u - F), X.reshape(n, C3 * P) * (0.5 / P)], 1)
    val64, idx64 = torch.from_numpy(g["edge_value"].astype(np.float64)), torch.from_numpy(g["edge_index"].astype(np.int64))
    ref, scale = bilinear_grads_f64(val64, idx64, n, theta + [0.0], nu, norm, bool(g["self_loops"]), V, W, stop="Q2")
    worst = check_theta(got, ref[:3], scale[:3], ["eps", "kappa", "outputscale"])
    RZ = sev.root_apply(Pi, Z)[0]
    rx = _rel_residual(Q, X.reshape(n, C3 * P), RZ.reshape(n, C3 * P))
    ry, ru = _rel3(RZ - _a64(p, Y), RZ), _rel3(gd[:, :, None] - _a64(p, u[:, :, None]), gd[:, :, None])
    # the probe term for the output scale (Q' = Q / scale) on the device's vectors against the dense trace
    dQ = Q / p["scale"]
    per = 0.5 * np.einsum("icp,icp->p", X, np.einsum("ij,jcp->icp", dQ, Y))
    exact = 0.5 * float((sev.trace_matrix(solver, Pi) * dQ).sum())
    est, se = float(per.mean()), float(per.std(ddof=1) / np.sqrt(P))
    total, terms, _ = sev.gradient(Q, dQ, F, p["t"], p["obs"], solver, gd)
    print("gradient (eps, kappa, outputscale) device %s, float64 on the device's vectors %s, worst %.4f of the bound; true residuals X "
          "%.2e, Y %.2e, u %.2e; output scale: probe term %.4f +- %.4f, dense trace %.4f (%.2f standard errors); dense analytic %.4f"
          % (["%.6f" % v for v in got], ["%.6f" % v for v in ref[:3]], worst, rx, ry, ru, est, se, exact, abs(est - exact) / se, total))
    assert max(rx, ry, ru) <= 2.0 * tol
    assert abs(est - exact) <= 4.0 * se
    assert abs(got[2] - (terms[0] + terms[1] + est)) <= 2e-4 * (abs(terms[0]) + abs(terms[1]) + np.abs(per).mean())
    plain = p["fit"].laplace_evidence(curvature=T(gd, dev))                                  # no operator: the value alone
    assert plain.solves is None and not plain.value.requires_grad
    assert abs(float(plain.value) - float(ev.value.detach())) <= DENSE_BAR * p["z"]["logdet"]         # the surrogate adds exactly 0


def test_sampled_curvature_is_within_its_standard_errors_of_the_dense_one(mgp, golden, dev):
    """softmax_sampled_curvature at 64 samples in blocks of 16 against the dense g.  E ||g - g_dense||^2 is the sum of the entries'
    variances, which ||se||^2 estimates from the same samples: the error's norm is within 3 of that of the standard errors (a ratio
    of 1 is expected; the 444 entries average the noise of the two norms).  Unobserved rows exactly 0; the same seed gives the
    same bits."""
    from manifold_gp_amd.evidence import softmax_sampled_curvature
    p = _problem(mgp, golden, dev, "dumbbell_k10_loop", "symmetric", 2)
    gd = sev.curvature(p["solver"], p["Pi"])
    g, se = softmax_sampled_curvature(p["fit"], 64, seed=5)
    gn, sn = g.cpu().numpy(), se.cpu().numpy()
    obs = p["obs"]
    ratio = np.linalg.norm((gn - gd)[obs]) / np.linalg.norm(sn[obs])
    print("sampled g, S = 64: ||error|| / ||se|| = %.3f, worst entry %.2f standard errors; ||error|| / ||g|| = %.3f"
          % (ratio, (np.abs(gn - gd)[obs] / sn[obs]).max(), np.linalg.norm((gn - gd)[obs]) / np.linalg.norm(gd[obs])))
    assert g.dtype == torch.float64 and g.shape == gd.shape and not gn[~obs].any() and not sn[~obs].any()
    assert ratio <= 3.0
    g2, _ = softmax_sampled_curvature(p["fit"], 64, seed=5)
    assert torch.equal(g, g2)


# ------------------------------------------------------------------------------------------------ 4: training, the model method
def _model(mgp, g, dev, y, kappa, scale, norm="symmetric", nu=2):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    x = T(g["train_x"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization=norm, num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=kappa)
    return RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, scale).to(dev)).to(dev), kern


def test_laplace_train_raises_the_dense_evidence(mgp, golden, dev):
    """laplace_train(family="multiclass") for 10 epochs of Adam(0.1) on the raw length scale and output scale from
    _evidence_ref.TRAIN's start, C = 3: the dense float64 log Z at the device run's end hyper-parameters exceeds the one at its start
    by at least half the gain of train_f64, the float64 run of the same optimiser with exact gradients (16.177;
    test_softmax_evidence_cpu.py reruns it)."""
    from manifold_gp_amd.utils import laplace_train
    tr = sev.TRAIN
    case, norm, nu = "dumbbell_k10_loop", "symmetric", 2
    g = golden(case)
    t, obs, y = sref.labels(g, C3)
    assert tr["gain_f64"] >= 5.0
    model, kern = _model(mgp, g, dev, T(y, dev), tr["kappa0"], tr["scale0"])
    kern.raw_graphbandwidth.requires_grad_(False)
    opt = torch.optim.Adam([kern.raw_lengthscale, model.covar_module.raw_outputscale], lr=tr["lr"])
    kappa0, scale0 = float(kern.lengthscale), float(model.covar_module.outputscale)
    last = laplace_train(model, opt, observed=T(obs, dev), family="multiclass", max_iter=tr["steps"] - 1, tolerance=0.0,
                         fit_kw=dict(num_classes=C3), evidence_kw=dict(var_samples=64))
    kappa1, scale1 = float(kern.lengthscale), float(model.covar_module.outputscale)

    def dense(kappa, scale):
        Q = eref.dense_q(g, norm, nu, float(g["eps"]), kappa, scale).numpy()
        Q = 0.5 * (Q + Q.T)
        solver = sref.Solver(Q, obs)
        return sev.log_z(Q, sref.newton(Q, t, obs, C3, solver=solver)[0], t, obs, solver)["value"]
    z0, z1 = dense(kappa0, scale0), dense(kappa1, scale1)
    print("laplace_train: float64 run gains %.3f; device run %.4f -> %.4f (gain %.3f; kappa %.4f -> %.4f, scale %.5g -> %.5g), last "
          "loss %.5f" % (tr["gain_f64"], z0, z1, z1 - z0, kappa0, kappa1, scale0, scale1, last))
    assert abs(kappa0 - tr["kappa0"]) <= 1e-6 * tr["kappa0"] and abs(scale0 - tr["scale0"]) <= 1e-5 * tr["scale0"]
    assert np.isfinite(last)
    assert z1 - z0 >= 0.5 * tr["gain_f64"]


def test_model_method_agrees_with_the_fit(mgp, golden, dev):
    from manifold_gp_amd.evidence import LaplaceEvidence, laplace_evidence
    g = golden("dumbbell_k10_loop")
    t, obs, y = sref.labels(g, C3)
    observed = T(obs, dev)
    model, kern = _model(mgp, g, dev, T(y, dev), float(g["kappa"]), 1.1e-5)
    c = model.laplace_evidence(observed=observed, family="multiclass", num_classes=C3, method="slq", seed=11, rtol=1e-5, var_samples=16)
    assert isinstance(c, LaplaceEvidence) and c.value.requires_grad and c.solves is not None and c.solves["g_se"] is not None
    grads = torch.autograd.grad(c.value, [kern.raw_lengthscale, model.covar_module.raw_outputscale])
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in grads)
    with torch.no_grad():
        a = model.laplace_evidence(observed=observed, family="multiclass", num_classes=C3, method="slq", seed=11, rtol=1e-5)
        fit = model.laplace_posterior_multiclass(C3, observed=observed, rtol=1e-5)
        b = fit.laplace_evidence(method="slq", seed=11)
        assert a.method == "slq" and a.se > 0.0 and not a.value.requires_grad and a.m == int(obs.sum())
        assert abs(float(a.value) - float(b.value)) <= 1e-6 * abs(float(b.value)) and a.per_probe.shape == (16,)
        e = model.laplace_evidence(observed=observed, family="multiclass", max_iter=4000, fit_kw=dict(num_classes=C3, rtol=1e-5),
                                   evidence_kw=dict(method="slq", seed=11, max_iter=3000))
        assert abs(float(e.value) - float(a.value)) <= 1e-6 * abs(float(a.value))
        with pytest.raises(ValueError, match="num_classes"):
            model.laplace_evidence(observed=observed, family="multiclass")
        with pytest.raises(TypeError):
            model.laplace_evidence(observed=observed, family="multiclass", num_classes=C3, evidence_kw=dict(rtol=1e-5))
    assert abs(float(c.value.detach()) - float(a.value)) <= 1e-3 * abs(float(a.value))       # the surrogate adds exactly 0
    with pytest.raises(NotImplementedError, match="laplace_evidence"):
        fit.evidence()
    with pytest.raises(NotImplementedError):
        laplace_evidence(fit)
    with pytest.raises(ValueError, match="family"):
        model.laplace_evidence(observed=observed, family="softmax")
