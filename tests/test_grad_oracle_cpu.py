"""The float64 gradient oracle (oracle/grad_ref.py) pinned on the CPU, with no GPU: its sparse model apply against the dense
differentiable model precision (oracle/ref_torch.py::dense_model_precision, itself pinned on the reference-autograd goldens), its
forward-mode tangent against a complex step, and the golden eps-gradients the reference's dense operators produced."""
import numpy as np
import pytest
import torch

from oracle.grad_ref import NAMES, laplacian_f64, laplacian_tangent_f64, model_apply_f64, underflow_eps
from oracle.ref_torch import dense_model_precision

CASES = ["dumbbell_k50_noloop", "dumbbell_k10_loop"]
NORMS = ["symmetric", "randomwalk"]


def _graph(golden, case):
    g = golden(case)
    return g, g["edge_value"], g["edge_index"].astype(np.int64), g["train_x"].shape[0], bool(g["self_loops"])


def _theta(g):
    return [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in (g["eps"], g["kappa"], 0.7, 1e-3)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_model_apply_matches_dense_model_precision(golden, case, norm, nu):
    """<W, Q3 V> and its gradients wrt eps, kappa, outputscale, noise: the sparse oracle against the dense one, 1e-10 relative
    (measured worst: 1.0e-14 on the values, 1.4e-14 on the gradients)."""
    g, val, idx, n, loops = _graph(golden, case)
    gen = torch.Generator().manual_seed(7 + nu)
    V = torch.randn(n, 2, generator=gen, dtype=torch.float64)
    W = torch.randn(n, 2, generator=gen, dtype=torch.float64)
    th = _theta(g)
    got = (W * model_apply_f64(val, idx, n, *th, nu, norm, loops, V)).sum()
    ggot = torch.autograd.grad(got, th)
    th2 = _theta(g)
    A = dense_model_precision(val, idx, n, *th2, nu, norm, loops)
    want = (W * (A @ V)).sum()
    gwant = torch.autograd.grad(want, th2)
    assert abs(float(got.detach() - want.detach())) <= 1e-10 * abs(float(want)), (float(got), float(want))
    for a, b in zip(ggot, gwant):
        assert abs(float(a - b)) <= 1e-10 * abs(float(b)), (float(a), float(b))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("bw", ["x0.25", "x1", "x4", "underflow"])
def test_tangent_matches_complex_step(golden, case, bw):
    """The jvp tangent of the six Laplacian arrays against Im f(eps + i h) / h with h = 1e-30 (no subtraction: exact to
    float64 rounding), to 1e-10 of each array's largest magnitude (measured worst: 3.4e-13), at the fixture's bandwidth, a
    quarter and four times of it, and at one where most weights underflow float32 (self loops on)."""
    g, val, idx, n, loops = _graph(golden, case)
    if bw == "underflow":
        eps, loops = underflow_eps(val), True
    else:
        eps = float(g["eps"]) * float(bw[1:])
    _, tan, scale, _ = laplacian_tangent_f64(val, idx, n, eps, loops)
    h = 1e-30
    cs = laplacian_f64(val, idx, n, torch.tensor(complex(eps, h), dtype=torch.complex128), loops)
    for k in NAMES:
        ref = cs[k].imag / h
        assert torch.isfinite(tan[k]).all() and torch.isfinite(scale[k]).all()
        assert float((tan[k] - ref).abs().max()) <= 1e-10 * float(ref.abs().max()), k
        assert bool((scale[k] >= 0).all())


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("norm", NORMS)
def test_golden_eps_gradients(golden, case, norm):
    """The reference's own float64 autograd (tests/golden: d/d eps of sum(L^T y) and of sum(P . L P)) reproduced by the
    oracle to 1e-8 relative (measured worst: 1.3e-15).  The goldens were taken at the decimal bandwidth (0.05, 0.5) that the
    fixture stores rounded to float32: its shortest repr gives it back.  Random walk without self loops has L 1 = 0, so
    sum(L^T y) is zero and its golden gradient is round-off (1e-13): "relative" there means relative to the sum of the
    magnitudes of the summed terms, sum_i |d (L^T y)_i / d eps|."""
    g, val, idx, n, loops = _graph(golden, case)
    p = norm + "_"
    y = torch.from_numpy(g["train_y"].astype(np.float64))
    P = torch.from_numpy(g["probes"].astype(np.float64))
    eps = float(str(g["eps"]))
    e = torch.tensor(eps, dtype=torch.float64, requires_grad=True)
    one = torch.ones((), dtype=torch.float64)

    def lty(x):
        return model_apply_f64(val, idx, n, x, one, one, one, 1, norm, loops, y.view(-1, 1), transposed=True, stop="L")
    _, d = torch.func.jvp(lty, (e.detach(),), (one,))
    got, terms = float(d.sum()), float(d.abs().sum())
    ref = float(g[p + "grad_eps_sum_LTv"])
    assert abs(got - ref) <= 1e-8 * max(abs(ref), terms), (got, ref, terms)
    e_ltv = abs(got - ref) / max(abs(ref), terms)
    e = torch.tensor(eps, dtype=torch.float64, requires_grad=True)
    q = (P * model_apply_f64(val, idx, n, e, one, one, one, 1, norm, loops, P, stop="L")).sum()
    got = torch.autograd.grad(q, e)[0].item()
    ref = float(g[p + "grad_eps_quadform"])
    assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)
    print("golden eps gradients %s %s: rel err %.1e, %.1e" % (case, norm, e_ltv, abs(got - ref) / abs(ref)))


def test_value_term_scale_closed_form_and_bounds_the_values(golden):
    """laplacian_value_scale_f64 on a two-node graph with one edge, against the closed form (a weight W = exp(-q), q = d2 / (4
    eps^2), counts as m = W (1 + q); every node has D~ = 1 + W, so s_D~ = 1 + m, s_A = m / D~^2 (1 + 2 s_D~ / D~), s_D = s_A +
    (1 + 2 s_D~ / D~) / D~^2, s_S = (s_A + A s_D / D) / (D eps^2) with A counted as m / D~^2); and on a golden graph: scale +
    floor bounds every value, the floor is zero where no weight underflows float32 and positive where most do, and the values
    are those of laplacian_tangent_f64."""
    from oracle.grad_ref import VALUE_NAMES, laplacian_value_scale_f64
    d2, eps = 0.3, 0.4
    value, scale, floor = laplacian_value_scale_f64(torch.tensor([d2], dtype=torch.float64), torch.tensor([[0], [1]]), 2, eps, True)
    q = d2 / (4 * eps * eps)
    W = np.exp(-q)
    m, dt = W * (1 + q), 1 + W
    s_dt = 1 + m
    s_a = m / dt ** 2 * (1 + 2 * s_dt / dt)
    s_d = s_a + (1 + 2 * s_dt / dt) / dt ** 2
    D = (1 + W) / dt ** 2
    want = dict(w=m, degree_unnorm=s_dt, a=s_a, degree=s_d, dsqrt=0.5 * s_d / D ** 0.5, dinvsqrt=0.5 * s_d / D ** 1.5,
                triu=(s_a + m / dt ** 2 * s_d / D) / (D * eps * eps),
                diag=(2 * s_dt / (dt ** 3 * D) + s_d / (dt * D) ** 2 + 1 + 1 / (dt * dt * D)) / (eps * eps))
    assert set(want) == set(VALUE_NAMES)
    for k in VALUE_NAMES:
        assert abs(float(scale[k][0]) - want[k]) <= 1e-14 * want[k], k
        assert float(floor[k].abs().max()) == 0.0
    assert abs(float(value["degree"][0]) - D) <= 1e-15 and abs(float(value["a"][0]) - W / dt ** 2) <= 1e-15
    g, val, idx, n, loops = _graph(golden, "dumbbell_k10_loop")
    for eps in (float(g["eps"]), underflow_eps(val)):
        value, scale, floor = laplacian_value_scale_f64(val, idx, n, eps, loops)
        ref = laplacian_tangent_f64(val, idx, n, eps, loops)[0]
        for k in VALUE_NAMES:
            assert bool(torch.isfinite(scale[k]).all()) and bool((scale[k] >= 0).all()) and bool((floor[k] >= 0).all())
            half = 2.0 if k in ("dsqrt", "dinvsqrt") else 1.0       # D^(+-1/2) is moved by HALF the relative change of D
            assert bool((value[k].abs() <= half * (scale[k] + floor[k]) * (1 + 1e-12)).all()), (eps, k)
            if k in NAMES:
                assert torch.equal(value[k], ref[k])
        assert (float(floor["triu"].max()) == 0.0) == (eps == float(g["eps"]))


def test_tangent_term_scale_bounds_the_tangent(golden):
    """The term scale is a sum of magnitudes of the terms that make up each tangent entry, so it bounds the entry; the
    floor is zero where no weight underflows float32 and positive where the bandwidth is small enough that some do."""
    g, val, idx, n, loops = _graph(golden, "dumbbell_k10_loop")
    for eps in (float(g["eps"]), underflow_eps(val)):
        _, tan, scale, floor = laplacian_tangent_f64(val, idx, n, eps, loops)
        for k in NAMES:
            assert bool((tan[k].abs() <= (scale[k] + floor[k]) * (1 + 1e-12)).all()), (eps, k)
        if eps == float(g["eps"]):
            assert float(floor["triu"].max()) == 0.0
        else:
            assert float(floor["triu"].max()) > 0.0
