"""The six small entry points of csrc/features.hip, each called directly and compared entry by entry with the float64
restatement of tests/_spectral_ref.py on the same float32 inputs:

  mgp_eigvec_postprocess   mgp_features_insample   mgp_features_oos   (through _lib.lib(): they have no Python wrapper)
  mgp_kernel_diag          mgp_lowrank_apply       mgp_lowrank_residual   (through manifold_gp_amd.solvers)

Every call asserts: float32 output, finite, |got - want| <= bound, and the same bits from a second call.  The bound is the
derived one of _spectral_ref ((L + 16) 2^-24 S, exponentials weighted by 1 + |argument|; for mgp_lowrank_residual one fp32
rounding plus the double-precision sum); nothing in it comes from device output.  The structure cases (row counts past every grid
and partial-block cap) run on integer / dyadic inputs whose fp32 sums are exact in any order and compare at 2 ulp, so that a
dropped row block is an integer-sized error.  Refusals leave a NaN canary untouched.

Measured worst |got - want| / bound per kernel are recorded in the docstrings below and in docs/kernels/features.md.
"""
import numpy as np
import pytest
import torch

import _spectral_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3
WORST = {}


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


def _off(a, dev):
    """The array on the device one element off a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    t = T(np.concatenate([a.reshape(-1)[:1], a.reshape(-1)]), dev)[1:].view(a.shape)
    assert t.data_ptr() % 16 == (4 if a.dtype.itemsize == 4 else 8) and t.is_contiguous()
    return t


def _out(shape, dev, off=False):
    """A float32 output full of NaN (an entry nobody wrote, or a write after a refusal, shows)."""
    n = int(np.prod(shape))
    if off:
        t = torch.full((n + 1,), float("nan"), device=dev)[1:].view(*shape)
        assert t.data_ptr() % 16 == 4
        return t
    return torch.full(tuple(shape), float("nan"), device=dev)


def _check(kernel, got, want, bound, what):
    """float32, finite, within the bound entry by entry (exact where the bound is 0); returns and records the worst ratio."""
    assert got.dtype == torch.float32, (what, got.dtype)
    g = got.double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(g).all(), what
    err = np.abs(g - want)
    bad = err > bound
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(bound, 1e-300))[bad].max()),
                           np.argwhere(bad)[:4].tolist())
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    return worst


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: a second call gave other bits" % what


# ============================================================================= runners (each calls twice)
def run_postprocess(V, deg, dev, up=T):
    from manifold_gp_amd._lib import lib, ptr, stream
    n, m = V.shape
    outs = []
    for _ in range(2):
        Vd, dg = up(V, dev), up(deg, dev)
        nw = int(lib().mgp_eigvec_postprocess_work_floats(m))
        work = _out((nw,), dev, off=up is _off)
        assert lib().mgp_eigvec_postprocess(ptr(Vd), n, m, ptr(dg), ptr(work), stream()) == 0
        outs.append(Vd)
    _same_bits(outs[0], outs[1], "postprocess")
    return outs[0]


def run_insample(inp, nu, kappa, dev, up=T):
    from manifold_gp_amd._lib import lib, ptr, stream
    n, m = inp["V"].shape
    ev, V = up(inp["evals"], dev), up(inp["V"], dev)
    outs = []
    for _ in range(2):
        Z = _out((n, m), dev, off=up is _off)
        assert lib().mgp_features_insample(ptr(ev), ptr(V), n, m, nu, float(kappa), ptr(Z), stream()) == 0
        outs.append(Z)
    _same_bits(outs[0], outs[1], "insample")
    return outs[0]


def _oos_call(lib_, a, n, m, nu, kappa, inp, norm, Tn, k, Z):
    from manifold_gp_amd._lib import ptr, stream
    return lib_.mgp_features_oos(ptr(a["evals"]), ptr(a["V"]), n, m, nu, float(kappa), float(inp["eps"]), norm, ptr(a["dtil"]),
                                 ptr(a["deg"]), ptr(a["d2"]), ptr(a["idx"]), Tn, k, float(inp["bump_scale"]),
                                 float(inp["bump_decay"]), ptr(Z), stream())


def run_oos(inp, nu, kappa, norm, dev, up=T, finite=True):
    from manifold_gp_amd._lib import lib
    n, m = inp["V"].shape
    Tn, k = inp["idx"].shape
    a = {key: up(inp[key], dev) for key in ("evals", "V", "dtil", "deg", "d2", "idx")}
    outs = []
    for _ in range(2):
        Z = _out((Tn, m), dev, off=up is _off)
        assert _oos_call(lib(), a, n, m, nu, kappa, inp, norm, Tn, k, Z) == 0
        outs.append(Z)
    _same_bits(outs[0], outs[1], "oos")
    return outs[0]


def _oos_ref(inp, nu, kappa, norm):
    inside = R.support_f32(inp["d2"], inp["eps"], inp["bump_scale"])
    return R.oos(inp["evals"], inp["V"], nu, kappa, inp["eps"], norm, inp["dtil"], inp["deg"], inp["d2"], inp["idx"],
                 inp["bump_scale"], inp["bump_decay"], inside), inside


def run_residual(Z, Tm, V, scale, dev, up=T):
    from manifold_gp_amd._lib import lib, ptr, stream
    n, m = Z.shape
    C = Tm.shape[1]
    Zd, Td, Vd = up(Z, dev), up(Tm, dev), up(V, dev)
    assert Td.dtype == torch.float64
    outs = []
    for _ in range(2):
        out = _out((n, C), dev, off=up is _off)
        assert lib().mgp_lowrank_residual(ptr(Zd), n, m, ptr(Td), ptr(Vd), C, float(scale), ptr(out), stream()) == 0
        outs.append(out)
    _same_bits(outs[0], outs[1], "residual")
    return outs[0]


def run_diag(Z1, Z2, scale, dev):
    from manifold_gp_amd.solvers import kernel_diag
    a, b = T(Z1, dev), T(Z2, dev)
    o1, o2 = kernel_diag(a, b, scale), kernel_diag(a, b, scale)
    _same_bits(o1, o2, "kernel_diag")
    return o1


def run_apply(Z, X, alpha, beta, dev):
    from manifold_gp_amd.solvers import lowrank_apply
    a, b = T(Z, dev), T(X, dev)
    o1, o2 = lowrank_apply(a, b, alpha, beta), lowrank_apply(a, b, alpha, beta)
    _same_bits(o1, o2, "lowrank_apply")
    return o1


# ============================================================================= mgp_eigvec_postprocess
@pytest.mark.parametrize("n,m", [(1025, m) for m in (1, 3, 4, 100, 256, 257, 513, 1024)] + [(n, 5) for n in (1, 255, 1024, 1025)])
def test_postprocess_vs_float64(mgp, dev, n, m):
    """Random eigenvectors and degrees in [0.2, 5]: every entry within (n + 17) 2^-24 of its float64 value; column 0 (when
    there is more than one) is all zero, where the 1e-12 clamp applies and the output is exactly 0.
    Measured worst ratio: 0.056 (n = 1, m = 5); 0.013 at n >= 255."""
    rng = np.random.default_rng([n, m])
    V = rng.standard_normal((n, m)).astype(np.float32)
    if m > 1:
        V[:, 0] = 0.0
    deg = rng.uniform(0.2, 5.0, n).astype(np.float32)
    want, bound = R.postprocess(V, deg)
    got = run_postprocess(V, deg, dev)
    worst = _check("eigvec_postprocess", got, want, bound, (n, m))
    if m > 1:
        assert float(got[:, 0].abs().max()) == 0.0 and float(bound[:, 0].max()) == 0.0
    print("postprocess n=%d m=%d: worst ratio %.3f" % (n, m, worst))


# ============================================================================= mgp_features_insample
@pytest.mark.parametrize("n,m", [(37, m) for m in R.INSAMPLE_M] + [(1025, 513)])
def test_insample_vs_float64(mgp, dev, n, m):
    """nu in {1, 2, 3} x kappa in {0.05, 0.5, 20}, eigenvalues 0 ... 1600: every entry within (m + 17) 2^-24 (1 + nu)^2 of its
    float64 value.  n m = 525,825 at (1025, 513) is past the 2048 x 256 grid (grid-stride loop)."""
    inp = R.insample_inputs(n, m)
    if (n, m) == (1025, 513):
        assert n * m > 2048 * 256
    worst = 0.0
    for nu in R.INSAMPLE_NU:
        for kappa in R.INSAMPLE_KAPPA:
            want, bound = R.insample(inp["evals"], inp["V"], nu, kappa)
            worst = max(worst, _check("features_insample", run_insample(inp, nu, kappa, dev), want, bound, (n, m, nu, kappa)))
    print("insample n=%d m=%d: worst ratio %.3f" % (n, m, worst))


def test_insample_refuses_more_than_1024_modes(mgp, dev):
    from manifold_gp_amd._lib import lib, ptr, stream
    inp = R.insample_inputs(3, 1025)
    Z = _out((3, 1025), dev)
    assert lib().mgp_features_insample(ptr(T(inp["evals"], dev)), ptr(T(inp["V"], dev)), 3, 1025, 1, 0.5, ptr(Z), stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(Z).all()), "a refused call must leave Z untouched"


# ============================================================================= mgp_features_oos
@pytest.mark.parametrize("shape", R.OOS_SHAPES, ids=lambda s: "n%d_m%d_T%d_k%d" % s)
def test_oos_vs_float64(mgp, dev, shape):
    """Hand-built neighbour lists (distinct ids, 0 and n - 1 among them, d2 ascending), arbitrary positive degree arrays, both
    normalisations, nu in {1, 2, 3}: every entry within (3 k + m + 17) 2^-24 S, S the float64 sum of the entry's terms in
    magnitude with each exponential weighted by 1 + |argument|."""
    inp = R.oos_inputs(*shape)
    n, m, Tn, k = shape
    assert inp["idx"].min() == 0 and inp["idx"].max() == n - 1
    assert all(len(set(row.tolist())) == k for row in inp["idx"][:8])
    worst = 0.0
    for norm in (0, 1):
        for nu in (1, 2, 3):
            (want, bound), inside = _oos_ref(inp, nu, 0.5, norm)
            assert inside.all()
            worst = max(worst, _check("features_oos", run_oos(inp, nu, 0.5, norm, dev), want, bound, (shape, norm, nu)))
    print("oos %r: worst ratio %.3f" % (shape, worst))


@pytest.mark.parametrize("norm", [0, 1])
def test_oos_support_edge(mgp, dev, norm):
    """One batch over the edge of the bump support (eps = 0.5, bump scale 4: alpha = 2, every number representable): a test
    point on a node (d = 0) and one at alpha / 2 meet the accuracy bound; one exactly at alpha (d2 = 4) and one far outside
    (weights exp(-2500): all underflow) are exactly 0.0, not NaN."""
    inp = R.oos_edge_inputs()
    (want, bound), inside = _oos_ref(inp, 2, 0.5, norm)
    assert inside.tolist() == [True, True, False, False]
    assert float(np.abs(want[:2]).min()) > 0.0
    got = run_oos(inp, 2, 0.5, norm, dev)
    _check("features_oos", got, want, bound, ("edge", norm))
    assert float(got[2:].abs().max()) == 0.0 and not bool(torch.isnan(got).any())


@pytest.mark.parametrize("norm", [0, 1])
def test_oos_underflowing_weights_give_the_float32_nan_pattern(mgp, dev, norm):
    """An in-support row whose k weights all underflow float32 has test degree 0: 0 / 0.  The reference's float32 arithmetic
    does the same; the kernel's NaN pattern equals that of a float32 numpy restatement (a whole row of NaN), and the
    ordinary row next to it meets the accuracy bound (include/mgp_hip.h states the behaviour)."""
    from manifold_gp_amd._lib import lib
    inp = R.oos_underflow_inputs()
    n, m = inp["V"].shape
    Tn, k = inp["idx"].shape
    pattern = R.oos_nan_pattern_f32(inp["evals"], inp["V"], 1, 0.5, inp["eps"], norm, inp["dtil"], inp["deg"], inp["d2"],
                                    inp["idx"], inp["bump_scale"], inp["bump_decay"])
    assert pattern[1].all() and not pattern[0].any()
    a = {key: T(inp[key], dev) for key in ("evals", "V", "dtil", "deg", "d2", "idx")}
    Z = _out((Tn, m), dev)
    assert _oos_call(lib(), a, n, m, 1, 0.5, inp, norm, Tn, k, Z) == 0
    assert np.array_equal(torch.isnan(Z).cpu().numpy(), pattern)
    (want, bound), inside = _oos_ref(inp, 1, 0.5, norm)
    assert inside.all()
    _check("features_oos", Z[:1], want[:1], bound[:1], ("underflow, ordinary row", norm))


def test_oos_refusals(mgp, dev):
    """k = 1025 and normalisation 2 return MGP_ERR_ARG (so does m = 1025) and leave Z untouched."""
    from manifold_gp_amd._lib import lib
    inp = R.oos_inputs(1037, 3, 2, 2)
    a = {key: T(inp[key], dev) for key in ("evals", "V", "dtil", "deg", "d2", "idx")}
    wide = dict(a, d2=torch.zeros(2, 1025, device=dev), idx=torch.zeros(2, 1025, dtype=torch.int32, device=dev))
    many = dict(a, evals=torch.zeros(1025, device=dev), V=torch.zeros(1037, 1025, device=dev))
    for args, m, k, norm in ((wide, 3, 1025, 0), (a, 3, 2, 2), (a, 3, 2, -1), (many, 1025, 2, 0)):
        Z = _out((2, m), dev)
        assert _oos_call(lib(), args, 1037, m, 1, 0.5, inp, norm, 2, k, Z) == ERR_ARG, (m, k, norm)
        torch.cuda.synchronize()
        assert bool(torch.isnan(Z).all())


@pytest.fixture(scope="module")
def golden_operator(mgp, golden, dev):
    """GraphLaplacianOperator of the 1,546-node fixture per normalisation, its test neighbour lists, and a float64
    oracle.laplacian twin that holds the operator's own float32 degree arrays (the kernel's inputs) upcast."""
    from oracle.laplacian import LaplacianOracle
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    idx, val = T(g["edge_index"].astype(np.int64), dev), T(g["edge_value"], dev)
    out = {}
    for norm in ("symmetric", "randomwalk"):
        eps = torch.tensor(float(g["eps"]), device=dev)
        op = mgp.operators.GraphLaplacianOperator(val, idx, n, eps.view(1, 1), norm, bool(g["self_loops"]), False)
        d = op.data
        lo = LaplacianOracle(g["edge_value"], g["edge_index"], n, R.f32(d.eps), norm, bool(g["self_loops"]), dtype=np.float64)
        lo.degree_unnorm = d.degree_unnorm.double().cpu().numpy()
        lo.degree = d.degree.double().cpu().numpy()
        out[norm] = (op, lo)
    return g, out


@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
@pytest.mark.parametrize("cols", [1, 5, 1024, 1025])
def test_constant_density_call_vs_oracle_out_of_sample(mgp, dev, golden_operator, norm, cols):
    """GraphLaplacianOperator.out_of_sample (zero eigenvalues, infinite support, decay 0: the kernel's Nystrom extension
    alone) against oracle.laplacian's float64 out_of_sample on the same degree arrays, at the features_oos bound times the
    sqrt(m / N) the wrapper undoes, plus one rounding for that product.  1,025 columns are more than the kernel's 1024 modes:
    the wrapper splits them into chunks and undoes the factor per chunk."""
    g, ops = golden_operator
    op, lo = ops[norm]
    n = op.operator_dimension
    d2, idx = g["knn_test_D"].astype(np.float32), g["knn_test_I"].astype(np.int32)
    x = np.random.default_rng(cols).standard_normal((n, cols)).astype(np.float32)
    want = lo.out_of_sample(x.astype(np.float64), d2.astype(np.float64), idx.astype(np.int64))
    bound = np.empty_like(want)
    for c0 in range(0, cols, 1024):
        xc = x[:, c0:c0 + 1024]
        mc = xc.shape[1]
        with np.errstate(over="ignore"):
            bs = float(np.float32(3.0e38 / max(op.data.eps, 1e-30)))      # what the wrapper passes: +inf at eps < 0.88
        w2, b2 = R.oos(np.zeros(mc, np.float32), xc, 1, 1.0, op.data.eps, 0 if norm == "symmetric" else 1, lo.degree_unnorm,
                       lo.degree, d2, idx, bs, 0.0, np.ones(d2.shape[0], bool))
        f = (mc / float(n)) ** 0.5
        assert np.abs(w2 * f - want[:, c0:c0 + 1024]).max() <= 1e-12 * np.abs(want).max()     # the two float64 statements agree
        bound[:, c0:c0 + 1024] = b2 * f + R.U * np.abs(want[:, c0:c0 + 1024])
    got = op.out_of_sample(T(x, dev), T(d2, dev), T(idx.astype(np.int64), dev))
    assert tuple(got.shape) == want.shape
    worst = _check("features_oos", got, want, bound, (norm, cols))
    print("out_of_sample %s %d columns: worst ratio %.3f" % (norm, cols, worst))


# ============================================================================= mgp_kernel_diag
@pytest.mark.parametrize("m", [1, 15, 16, 17, 100, 1024])
@pytest.mark.parametrize("n", [1, 15, 17, 389])
def test_kernel_diag_vs_float64(mgp, dev, n, m):
    """Z1 != Z2, scale 1.7: every entry within (m + 17) 2^-24 |scale| sum_j |z1 z2|."""
    rng = np.random.default_rng([n, m, 1])
    Z1, Z2 = rng.standard_normal((n, m)).astype(np.float32), rng.standard_normal((n, m)).astype(np.float32)
    want, bound = R.kernel_diag(Z1, Z2, 1.7)
    worst = _check("kernel_diag", run_diag(Z1, Z2, 1.7, dev), want, bound, (n, m))
    print("kernel_diag n=%d m=%d: worst ratio %.3f" % (n, m, worst))


# ============================================================================= mgp_lowrank_apply
APPLY = [(1, 1, 1), (255, 3, 3), (517, 37, 4), (4096, 256, 1), (517, 257, 17), (255, 600, 3), (4096, 3, 17), (1, 600, 4),
         (4096, 37, 3)]


@pytest.mark.parametrize("n,m,C", APPLY)
def test_lowrank_apply_vs_float64(mgp, dev, n, m, C):
    """alpha Z (Z^T X) + beta X: every entry within (n + m + 18) 2^-24 (|alpha| |Z| (|Z|^T |X|) + |beta| |X|).  n = 4096 is 16
    row blocks of zt_x_partial; m = 257, 600 take more than one pass of its 256 column lanes."""
    rng = np.random.default_rng([n, m, C])
    Z, X = rng.standard_normal((n, m)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    want, bound = R.lowrank_apply(Z, X, 0.3, 0.2)
    worst = _check("lowrank_apply", run_apply(Z, X, 0.3, 0.2, dev), want, bound, (n, m, C))
    print("lowrank_apply n=%d m=%d C=%d: worst ratio %.3f" % (n, m, C, worst))


def test_lowrank_apply_one_dimensional_x(mgp, dev):
    rng = np.random.default_rng(5)
    Z, X = rng.standard_normal((517, 37)).astype(np.float32), rng.standard_normal(517).astype(np.float32)
    want, bound = R.lowrank_apply(Z, X[:, None], 0.3, 0.2)
    got = run_apply(Z, X, 0.3, 0.2, dev)
    assert got.dim() == 1
    _check("lowrank_apply", got, want[:, 0], bound[:, 0], "1-D X")


def test_lowrank_apply_refuses_a_short_workspace(mgp, dev):
    from manifold_gp_amd._lib import lib, ptr, stream
    n, m, C = 255, 37, 3
    Z, X = torch.randn(n, m, device=dev), torch.randn(n, C, device=dev)
    wb = int(lib().mgp_lowrank_workspace_bytes(m, C))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    Y = _out((n, C), dev)
    assert lib().mgp_lowrank_apply(ptr(Z), n, m, ptr(X), C, 0.3, 0.2, ptr(Y), ptr(work), wb - 1, stream()) == ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(Y).all()), "a refused call must leave Y untouched"
    assert lib().mgp_lowrank_apply(ptr(Z), n, m, ptr(X), C, 0.3, 0.2, ptr(Y), ptr(work), wb, stream()) == 0


# ============================================================================= mgp_lowrank_residual
@pytest.mark.parametrize("n,m,C", [(300, 1, 1), (300, 100, 1), (300, 299, 20), (37, 6144, 1), (3, 1, 6144)])
def test_lowrank_residual_vs_float64(mgp, dev, n, m, C):
    """scale (V - Z T), T float64: u |want| + (m + 4) 2^-53 |scale| sum |z t|.  m C = 6144 is the last size whose T fits the
    48 KiB of LDS."""
    rng = np.random.default_rng([n, m, C, 2])
    Z, V = rng.standard_normal((n, m)).astype(np.float32), rng.standard_normal((n, C)).astype(np.float32)
    Tm = rng.standard_normal((m, C))
    want, bound = R.lowrank_residual(Z, Tm, V, 100.0)
    worst = _check("lowrank_residual", run_residual(Z, Tm, V, 100.0, dev), want, bound, (n, m, C))
    print("lowrank_residual n=%d m=%d C=%d: worst ratio %.3f" % (n, m, C, worst))


def test_lowrank_residual_refuses_past_the_lds(mgp, dev):
    """(m, C) = (3, 2049): 49,176 bytes of T against 49,152 of LDS -> MGP_ERR_UNSUPPORTED before any launch."""
    from manifold_gp_amd._lib import lib, ptr, stream
    n, m, C = 5, 3, 2049
    Z, V = torch.randn(n, m, device=dev), torch.randn(n, C, device=dev)
    Tm = torch.randn(m, C, dtype=torch.float64, device=dev)
    out = _out((n, C), dev)
    assert lib().mgp_lowrank_residual(ptr(Z), n, m, ptr(Tm), ptr(V), C, 1.0, ptr(out), stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_lowrank_residual_cancelling(mgp, dev):
    """V = fp32(Z T) + 2^-20 noise: |want| is a millionth of |V| (asserted), the case the double-precision row sums are for --
    a float32 sum of the m = 100 terms would be off by ~ m 2^-24 |z||t| = 6e-6 |V|, several times |want| itself."""
    rng = np.random.default_rng(77)
    n, m, C = 1000, 100, 3
    Z = rng.standard_normal((n, m)).astype(np.float32)
    Tm = rng.standard_normal((m, C))
    V = ((Z.astype(np.float64) @ Tm).astype(np.float32) + np.float32(2.0 ** -20) * rng.standard_normal((n, C)).astype(np.float32))
    want, bound = R.lowrank_residual(Z, Tm, V, 100.0)
    assert np.median(np.abs(want) / 100.0) < 4e-6 * np.median(np.abs(V))
    worst = _check("lowrank_residual", run_residual(Z, Tm, V, 100.0, dev), want, bound, "cancelling")
    print("lowrank_residual cancelling: worst ratio %.3f" % worst)


def test_woodbury_gram_path_and_library_fallback_at_299_modes(mgp, dev):
    """woodbury at m = 299 with C = 20 (m C = 5980 <= 6144: Gram pass + mgp_lowrank_residual) and C = 21 (6279: library GEMMs)
    against the float64 solve at the 1e-4 of max |ref| that test_downstream_of_eval_at_299_modes holds it to; the two paths
    agree with each other on their 20 common columns within the same bar."""
    from manifold_gp_amd.solvers import woodbury
    n, m, s, noise = 2000, 299, 0.7, 1e-2
    gen = torch.Generator().manual_seed(299)
    Z = (torch.randn(n, m, generator=gen) / m ** 0.5).to(dev)
    Y = torch.randn(n, 21, generator=gen).to(dev)
    assert m + 20 <= 512 and m * 20 <= 6144 < m * 21
    Zd, Yd = Z.double(), Y.double()
    t = torch.linalg.solve(Zd.t() @ Zd + (noise / s) * torch.eye(m, device=dev, dtype=torch.float64), Zd.t() @ Yd)
    ref = (Yd - Zd @ t) / noise
    a20, a21 = woodbury(Z, Y[:, :20].contiguous(), s, noise)["alpha"], woodbury(Z, Y, s, noise)["alpha"]
    assert a20.dtype == torch.float32 and a21.dtype == torch.float32
    bar = 1e-4 * float(ref.abs().max())
    e20 = float((a20.double() - ref[:, :20]).abs().max())
    e21 = float((a21.double() - ref).abs().max())
    e2 = float((a20.double() - a21.double()[:, :20]).abs().max())
    print("woodbury m=299: Gram path %.2e, fallback %.2e, between the paths %.2e of max|ref|" % tuple(
        e / float(ref.abs().max()) for e in (e20, e21, e2)))
    assert e20 < bar and e21 < bar and e2 < bar, (e20, e21, e2, bar)


# ============================================================================= structure: past every cap, exact inputs
def test_structure_postprocess_past_256_chunks(mgp, dev):
    """(263,001, 5): 257 chunks of 1024 rows are capped to 256 of 1028, and n m is past the 4096 x 256 grid of scale_cols.
    The column sums of squares are exact (multiples of 1/16 below 2^24 units): the output is sqrt, reciprocal and product of
    exact numbers, within 2 ulp."""
    n, m = R.STRUCTURE[0][1]
    assert -(-n // 1024) > 256 and n * m > 4096 * 256
    inp = R.exact_inputs("postprocess", (n, m), 1)
    want, _ = R.postprocess(inp["V"], inp["deg"])
    _check("structure", run_postprocess(inp["V"], inp["deg"], dev), want, R.ulp2(want), "postprocess")


def test_structure_kernel_diag_past_65536_groups(mgp, dev):
    n, m = R.STRUCTURE[1][1]
    assert n > 4096 * 256 // 16
    inp = R.exact_inputs("kernel_diag", (n, m), 2)
    want, _ = R.kernel_diag(inp["Z1"], inp["Z2"], inp["scale"])
    _check("structure", run_diag(inp["Z1"], inp["Z2"], inp["scale"], dev), want, R.ulp2(want), "kernel_diag")


@pytest.mark.parametrize("shape", [R.STRUCTURE[2][1], R.STRUCTURE[3][1]])
def test_structure_lowrank_apply_past_512_blocks(mgp, dev, shape):
    """(131,381, 3, 2): 514 blocks of 256 rows are capped to 512 of 257; (65,553, 3, 2): n C is past the 65,536 groups of
    z_t_axpby.  t = Z^T X are exact integers, so are the outputs: a dropped partial block is an integer-sized error."""
    n, m, C = shape
    assert (-(-n // 256) > 512) if n > 100_000 else (n * C > 4096 * 256 // 16)
    inp = R.exact_inputs("apply", shape, 3)
    want, _ = R.lowrank_apply(inp["Z"], inp["X"], inp["alpha"], inp["beta"])
    _check("structure", run_apply(inp["Z"], inp["X"], inp["alpha"], inp["beta"], dev), want, R.ulp2(want), shape)


def test_structure_lowrank_residual_past_8192_blocks(mgp, dev):
    n, m, C = R.STRUCTURE[4][1]
    assert n * C > 8192 * 256
    inp = R.exact_inputs("residual", (n, m, C), 4)
    want, _ = R.lowrank_residual(inp["Z"], inp["T"], inp["V"], inp["scale"])
    _check("structure", run_residual(inp["Z"], inp["T"], inp["V"], inp["scale"], dev), want, R.ulp2(want), "residual")


# ============================================================================= alignment: every array one element off
def test_every_array_one_element_off_16_bytes(mgp, dev):
    """One case per kernel with every device array (inputs, outputs, scratch) starting 4 bytes past a 16-byte boundary (8 for
    the float64 T)."""
    from manifold_gp_amd._lib import lib, ptr, stream
    rng = np.random.default_rng(16)
    n, m = 255, 37
    V = rng.standard_normal((n, m)).astype(np.float32)
    deg = rng.uniform(0.2, 5.0, n).astype(np.float32)
    _check("eigvec_postprocess", run_postprocess(V, deg, dev, up=_off), *R.postprocess(V, deg), "off")
    inp = R.insample_inputs(n, m)
    _check("features_insample", run_insample(inp, 2, 0.5, dev, up=_off), *R.insample(inp["evals"], inp["V"], 2, 0.5), "off")
    inp = R.oos_inputs(300, 100, 257, 10)
    (want, bound), _ = _oos_ref(inp, 2, 0.5, 0)
    _check("features_oos", run_oos(inp, 2, 0.5, 0, dev, up=_off), want, bound, "off")
    Z1, Z2 = V, rng.standard_normal((n, m)).astype(np.float32)
    out = _out((n,), dev, off=True)
    assert lib().mgp_kernel_diag(ptr(_off(Z1, dev)), ptr(_off(Z2, dev)), n, m, 1.7, ptr(out), stream()) == 0
    _check("kernel_diag", out, *R.kernel_diag(Z1, Z2, 1.7), "off")
    X = rng.standard_normal((n, 3)).astype(np.float32)
    Y = _out((n, 3), dev, off=True)
    wb = int(lib().mgp_lowrank_workspace_bytes(m, 3))
    work = torch.empty(wb + 16, dtype=torch.uint8, device=dev)[4:]
    assert work.data_ptr() % 16 == 4
    assert lib().mgp_lowrank_apply(ptr(_off(V, dev)), n, m, ptr(_off(X, dev)), 3, 0.3, 0.2, ptr(Y), ptr(work), wb, stream()) == 0
    _check("lowrank_apply", Y, *R.lowrank_apply(V, X, 0.3, 0.2), "off")
    Tm = rng.standard_normal((m, 3))
    _check("lowrank_residual", run_residual(V, Tm, X, 100.0, dev, up=_off), *R.lowrank_residual(V, Tm, X, 100.0), "off")


def test_worst_ratios_are_reported(mgp, dev):
    """Prints the worst |got - want| / bound of this run per kernel (pytest -s).  Measured on the MI355X:
    eigvec_postprocess 0.056, features_insample 0.037, features_oos 0.011, kernel_diag 0.091, lowrank_apply 0.0085,
    lowrank_residual 0.997 (its bound is one float32 rounding of the result, and a correct rounding reaches it), structure 0.45
    of the 2-ulp bar."""
    for k in sorted(WORST):
        print("worst ratio %-20s %.4f" % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())
