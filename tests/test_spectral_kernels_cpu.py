"""tests/_spectral_ref.py pinned without a GPU: its float64 restatement equals oracle/spectral.py and the committed float64
goldens, and every input set of tests/test_gpu_spectral_kernels.py has the properties its bounds rest on."""
import numpy as np
import pytest

import _spectral_ref as R
from oracle import spectral as osp
from oracle.laplacian import LaplacianOracle

CASES = ["dumbbell_k50_noloop", "dumbbell_k10_loop"]
NORMS = ["symmetric", "randomwalk"]
FLT_MAX = float(np.finfo(np.float32).max)


def _random_graph(n, rng, eps, norm, loops):
    r, c = np.triu_indices(n, 1)
    keep = rng.random(r.size) < 0.2
    idx = np.stack([r[keep], c[keep]])
    val = rng.uniform(0.05, 1.5, idx.shape[1])
    return LaplacianOracle(val, idx, n, eps, norm, loops, dtype=np.float64)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_restatement_equals_the_oracle(norm, nu):
    """insample, oos and postprocess against oracle.spectral on a random 60-node graph (eps, kappa, bump scale and decay
    representable in float32, so that the restatement's rounding of its scalars changes nothing): 1e-13 of the largest entry."""
    rng = np.random.default_rng([3, nu])
    n, m, Tn, k, eps, kappa, bs, bd = 60, 9, 12, 6, 0.5, 0.75, 4.0, 1.5
    lap = _random_graph(n, rng, eps, norm, True)
    w, U = np.linalg.eigh(lap.dense_symmetric())
    lam, Phi = osp.eval_eigenpairs(lap, m)
    got, _ = R.postprocess(U[:, :m], lap.degree)
    assert np.abs(got - Phi).max() <= 1e-13 * np.abs(Phi).max()
    want = osp.features_insample(lam, Phi, nu, kappa)
    got, bound = R.insample(lam, Phi, nu, kappa)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max() and (bound >= 0).all()
    idx = R.neighbour_lists(n, Tn, k, rng)
    # nearest distances from 0 to sqrt(6) = 2.45: some rows outside alpha = 2
    d2 = np.sort(rng.uniform(0.0, 1.0, (Tn, k)), axis=1) + np.linspace(0.0, 6.0, Tn)[:, None]
    inside = R.support_f64(d2, eps, bs)
    assert 0 < inside.sum() < Tn
    want = osp.features_oos(lap, lam, Phi, nu, kappa, d2, idx.astype(np.int64), bs, bd)
    got, bound = R.oos(lam, Phi, nu, kappa, eps, 0 if norm == "symmetric" else 1, lap.degree_unnorm, lap.degree, d2, idx, bs, bd,
                       inside)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert (got[~inside] == 0).all() and (bound[~inside] == 0).all() and (bound[inside] > 0).all()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("norm", NORMS)
def test_restatement_reproduces_the_float64_goldens(golden, case, norm):
    """postprocess -> insample on the float64 eigenpairs of the golden graph (the goldens store no eigenvectors: a float64 eigh
    of the oracle's L_sym, as eval_eigenpairs takes it) reproduce *_features_gram_64_f64 and *_features_diag_f64; oos the
    un-bumped extension Gram *_oos_gram_f64 -- at the tolerances tests/test_oracle_golden.py holds the oracle to."""
    g = golden(case)
    p = norm + "_"
    m, nu = int(g["modes"]), 1
    lap = LaplacianOracle(g["edge_value"], g["edge_index"], g["train_x"].shape[0], float(g["eps"]), norm, bool(g["self_loops"]),
                          dtype=np.float64)
    kappa = float(g["kappa"])
    assert R.f32(kappa) == kappa and R.f32(lap.eps) == float(lap.eps)           # the fixture stores them as float32
    w, U = np.linalg.eigh(lap.dense_symmetric())
    lam = w[:m].copy()
    lam[0] = 0.0
    Phi, _ = R.postprocess(U[:, :m], lap.degree)
    Z, _ = R.insample(lam, Phi, nu, kappa)
    ref = g[p + "features_gram_64_f64"]
    assert np.abs(Z[:64] @ Z[:64].T - ref).max() <= 1e-8 * np.abs(ref).max()
    np.testing.assert_allclose((Z * Z).sum(-1), g[p + "features_diag_f64"], rtol=1e-8)
    bs, bd = float(g["bump"][0]), float(g["bump"][1])
    d2, idx = g["knn_test_D"].astype(np.float64), g["knn_test_I"].astype(np.int64)
    inside = R.support_f64(d2, lap.eps, bs)
    Zt, _ = R.oos(lam, Phi, nu, kappa, lap.eps, 0 if norm == "symmetric" else 1, lap.degree_unnorm, lap.degree, d2, idx,
                  R.f32(bs), R.f32(bd), inside)
    b, _ = R.bump(d2[:, 0], lap.eps, bs, bd)
    assert inside.any()
    ext = (Zt[inside] / b[inside, None]) @ Z[:64].T
    ref = g[p + "oos_gram_f64"]
    assert np.abs(ext - ref[inside]).max() <= 1e-8 * np.abs(ref).max()


# ------------------------------------------------------------------------------ what the GPU file's bounds rest on
def _normal(x):
    x = np.abs(np.asarray(x, np.float64))
    return bool(((x >= R.FLT_MIN) & (x <= FLT_MAX)).all())


def _oos_sets(golden):
    for name, inp in R.all_oos_inputs():
        yield name, inp, True
    yield "underflow", R.oos_underflow_inputs(), False
    g = golden("dumbbell_k10_loop")
    eps = float(g["eps"])
    # the wrapper's "infinite support": 3e38 / eps is past float32 and arrives as +inf
    yield "constant density", dict(d2=g["knn_test_D"].astype(np.float32), eps=eps, bump_scale=float("inf"),
                                   evals=np.zeros(5, np.float32)), True


def test_support_decisions_agree_and_weights_are_normal(golden):
    """For every features_oos input set: the float32 and the float64 support decision agree row by row; every in-support
    row's largest weight is at least 2^-100, so the test degree is a normal float32 (the one exception is the row that pins the
    0 / 0 behaviour, whose largest weight is below 2^-126 on purpose); 1 - eps^2 lambda stays in [3/4, 1]."""
    seen = 0
    for name, inp, normal_weights in _oos_sets(golden):
        in32 = R.support_f32(inp["d2"], inp["eps"], inp["bump_scale"])
        in64 = R.support_f64(inp["d2"], inp["eps"], inp["bump_scale"])
        assert np.array_equal(in32, in64), name
        e = R.f32(inp["eps"])
        wmax = np.exp(-np.asarray(inp["d2"], np.float64) / (4.0 * e * e)).max(1)
        if normal_weights:
            assert (wmax[in32] >= 2.0 ** -100).all(), name
        else:
            assert in32.all() and wmax[1] < R.FLT_MIN and wmax[0] >= 2.0 ** -100, name
        t = 1.0 - e * e * np.asarray(inp["evals"], np.float64)
        assert (t >= 0.75).all() and (t <= 1.0).all(), name
        seen += 1
    assert seen == len(R.OOS_SHAPES) + 3
    edge = R.oos_edge_inputs()
    assert R.support_f32(edge["d2"], edge["eps"], edge["bump_scale"]).tolist() == [True, True, False, False]
    assert float(edge["d2"][2, 0]) == (edge["bump_scale"] * edge["eps"]) ** 2 == 4.0       # exactly on the edge


def test_spectral_density_sums_are_normal():
    """Every density s_j, their total and n s_j / total are normal float32 numbers, for every in-sample input set (nu x kappa)
    and every out-of-sample one (nu in {1, 2, 3}, kappa = 0.5, with the 1 / (1 - eps^2 lambda)^2 factor)."""
    for n, m in [(37, mm) for mm in R.INSAMPLE_M] + [(1025, 513), (3, 1025), (255, 37)]:
        lam = R.insample_inputs(n, m)["evals"]
        assert lam[0] == 0.0 and (np.diff(lam) > 0).all()
        assert m == 1 or abs(float(lam[-1]) - 4.0 / R.EPS_IN ** 2) < 1e-3
        for nu in R.INSAMPLE_NU:
            for kappa in R.INSAMPLE_KAPPA:
                sq, s, _ = R._sqrt_density(lam, nu, kappa, n)
                assert _normal(s) and _normal(s.sum()) and _normal(sq * sq), (n, m, nu, kappa)
    for name, inp in list(R.all_oos_inputs()) + [("underflow", R.oos_underflow_inputs())]:
        for nu in (1, 2, 3):
            sq, s, _ = R._sqrt_density(inp["evals"], nu, 0.5, inp["V"].shape[0], inp["eps"])
            assert _normal(s) and _normal(s.sum()) and _normal(sq * sq), (name, nu)


@pytest.mark.parametrize("kind,shape", R.STRUCTURE)
def test_exact_inputs_are_exact(kind, shape):
    """Every sum a kernel forms on `exact_inputs` data, evaluated in float32 front to back and back to front: both bit-equal
    to the float64 sum, and every magnitude below 2^24 units."""
    inp = R.exact_inputs(kind, shape, 1)
    sums = R.exact_sums(kind, inp)
    assert sums
    for fwd, bwd, ref in sums:
        assert fwd.dtype == np.float32 and bwd.dtype == np.float32
        assert np.array_equal(fwd.astype(np.float64), ref) and np.array_equal(bwd.astype(np.float64), ref)
        assert np.abs(ref).max() * (16 if kind == "postprocess" else 1) < 2.0 ** 24
    if kind in ("apply", "residual", "kernel_diag"):
        fn = dict(apply=lambda: R.lowrank_apply(inp["Z"], inp["X"], inp["alpha"], inp["beta"]),
                  residual=lambda: R.lowrank_residual(inp["Z"], inp["T"], inp["V"], inp["scale"]),
                  kernel_diag=lambda: R.kernel_diag(inp["Z1"], inp["Z2"], inp["scale"]))[kind]
        want = fn()[0]
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)       # the expected output is a float32 number
        assert np.abs(want).max() > 1.0
