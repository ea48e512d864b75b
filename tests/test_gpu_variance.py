"""Marginal posterior variances in precision form on the MI355X (csrc/variance.hip, sampling.posterior_variance): the exact
operator diagonal against the float64 matrix built from the device's own CSR, the row moments against numpy float64 on the
same float32 inputs, the estimator against its float64 restatement driven by the same Philox draws (tests/_variance_ref.py),
chunking, the plain method against the sampler, and the model methods."""
import ctypes

import numpy as np
import pytest
import torch

import _observed_ref as oref
import _variance_ref as vref

pytestmark = pytest.mark.gpu

FIXTURES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]
NORMS = ["symmetric", "randomwalk"]
SCALE = float(np.float32(1.3))          # the operator struct carries float32 scalars: references take the same values
NOISE = float(np.float32(1e-2))


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


def _desc(mgp, g, dev, norm, nu, scale=SCALE):
    idx = T(g["edge_index"].astype(np.int64), dev)
    val = T(g["edge_value"], dev)
    eps = torch.tensor([[float(g["eps"])]], device=dev)
    lap = mgp.operators.GraphLaplacianOperator(val, idx, g["train_x"].shape[0], eps, norm, bool(g["self_loops"]))
    kappa = torch.tensor([[float(g["kappa"])]], device=dev)
    return mgp.operators.PrecisionMaternOperator(lap, nu, kappa)._descriptor().with_(scale=scale)


def _noise_case(n, dev, per_node, seed=1):
    """(noise argument, observed argument, float64 variances, bool mask): a float noise with every node observed (form 2),
    or per-node variances from {1e-2, 4e-2} with 10 % of the nodes observed (form 3)."""
    if not per_node:
        return NOISE, None, np.full(n, NOISE), np.ones(n, bool)
    rng = np.random.default_rng(seed)
    var = rng.choice([1e-2, 4e-2], n).astype(np.float32)
    obs = rng.random(n) < 0.1
    return T(var, dev), T(obs, dev), var.astype(np.float64), obs


# ------------------------------------------------------------------------------------------------ the exact diagonal
@pytest.mark.parametrize("case", FIXTURES)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_diag_exact_matches_device_matrix(mgp, golden, dev, case, norm, nu):
    """forms 0, 2, 3 against the diagonal of the float64 Q2 of the device's own CSR (_observed_ref.device_q2) plus the form
    term: 1e-12 relative at every node; repeated calls are bitwise equal."""
    from manifold_gp_amd import sampling
    g = golden(case)
    desc = _desc(mgp, g, dev, norm, nu)
    n = desc.n
    q = oref.device_q2(desc).diagonal()
    rng = np.random.default_rng(nu)
    obs = rng.random(n) < 0.1
    s, w = oref.weights(rng.choice([1e-2, 4e-2], n).astype(np.float32), obs)
    s = float(np.float32(s))
    w32 = T(w.astype(np.float32), dev)
    w = w32.double().cpu().numpy()
    for form, d in ((0, desc), (2, desc.with_(form=2, noise=s)), (3, desc.with_(form=3, noise=s, obs_w=w32))):
        got = sampling.operator_diag_exact(d)
        assert got.dtype == torch.float64 and got.shape == (n,)
        want = vref.system_diag(q, form, s, w)
        rel = np.abs(got.cpu().numpy() / want - 1.0).max()
        print("form %d: worst node %.2e" % (form, rel))
        assert rel <= 1e-12, (form, rel)
        assert torch.equal(got, sampling.operator_diag_exact(d))


def test_diag_exact_refuses_nu_4_and_form_1(mgp, golden, dev):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    desc = _desc(mgp, golden("dumbbell_k10_loop"), dev, "symmetric", 4)
    out = torch.zeros(desc.n, dtype=torch.float64, device=dev)
    for d, want in ((desc.with_(form=2, noise=NOISE), -3), (desc.with_(nu=2, form=1, noise=NOISE), -3)):
        op = d.struct()
        assert lib.mgp_operator_diag_exact(ctypes.byref(op), _lib.ptr(out), None, 0, _lib.stream()) == want
    assert not out.any()


def _hand_graph(order):
    """Five nodes: the triangle 0-1-2, the pendant edge 2-3, the isolated node 4 whose row is padding only (col == row,
    S = 0).  Rows padded to four entries; order "ascending": columns ascend, padding at the row's end (what the graph
    builders write); "shuffled": entries and padding in another order (the linear look-up)."""
    rows = {0: [(1, 0.5), (2, 2.0)], 1: [(0, 0.5), (2, 0.25)], 2: [(0, 2.0), (1, 0.25), (3, 1.5)], 3: [(2, 1.5)], 4: []}
    col, val, rowptr = [], [], [0]
    for i in range(5):
        ent = rows[i] + [(i, 0.0)] * (4 - len(rows[i]))
        if order == "shuffled":
            ent = ent[::-1] if i != 2 else [ent[2], ent[3], ent[0], ent[1]]
        col += [c for c, _ in ent]
        val += [v for _, v in ent]
        rowptr.append(len(col))
    S_ = np.zeros((5, 5))
    for i in rows:
        for c, v in rows[i]:
            S_[i, c] = v
    return np.array(rowptr, np.int32), np.array(col, np.int32), np.array(val, np.float32), S_


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_diag_exact_hand_built_triangle(mgp, dev, order):
    """One triangle: the triangle term 2 S_01 S_12 S_20 sits at nodes 0, 1, 2 only; the padding-only row gives a_4^nu; the
    padding entries are skipped in either column order."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    rowptr, col, val, S_ = _hand_graph(order)
    diag = np.array([3.0, 4.0, 5.0, 6.0, 7.0], np.float32)
    pre = np.array([1.0, 0.5, 2.0, 1.5, 3.0], np.float32)
    w = np.array([1.0, 0.0, 0.25, 0.0, 0.5], np.float32)
    t = dict(rowptr=T(rowptr, dev), col=T(col, dev), val=T(val, dev), diag=T(diag, dev), pre=T(pre, dev), w=T(w, dev))
    kappa, scale, s = 2.0, 0.75, 0.125
    for nu in (1, 2, 3):
        tau = 2.0 * nu / kappa ** 2
        a = tau + diag.astype(np.float64)
        q = scale * pre.astype(np.float64) ** 2 * np.diag(np.linalg.matrix_power(np.diag(a) - S_, nu))
        if nu == 3:
            no_tri = a ** 3 + 2 * a * (S_ * S_).sum(1) + (S_ * S_) @ a
            assert np.allclose(no_tri - q / (scale * pre.astype(np.float64) ** 2), [0.5, 0.5, 0.5, 0, 0], atol=1e-12)
        for form in (0, 2, 3):
            op = _lib.OperatorT()
            op.L = _lib.csr_struct(5, t["rowptr"], t["col"], t["val"], t["diag"])
            op.pre = op.post = t["pre"].data_ptr()
            op.nu, op.kappa, op.scale, op.form, op.noise = nu, kappa, scale, form, s
            op.obs_w = t["w"].data_ptr() if form == 3 else None
            out = torch.empty(5, dtype=torch.float64, device=dev)
            _lib.check(lib.mgp_operator_diag_exact(ctypes.byref(op), _lib.ptr(out), None, 0, _lib.stream()), "diag_exact")
            want = vref.system_diag(q, form, s, w.astype(np.float64))
            assert np.abs(out.cpu().numpy() / want - 1.0).max() <= 1e-12, (nu, form, out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the row moments
def _moments(lib, U, V=None, rdiag=None, Pm=None, acc=None):
    from manifold_gp_amd import _lib
    n, C = U.shape
    acc = torch.zeros(n, 2, dtype=torch.float64, device=U.device) if acc is None else acc
    _lib.check(lib.mgp_row_moments(_lib.ptr(U), _lib.ptr(V), _lib.ptr(rdiag), _lib.ptr(Pm), n, C, _lib.ptr(acc),
                                   _lib.stream()), "mgp_row_moments")
    return acc


def _moments_ref(U, V=None, rdiag=None, Pm=None):
    """(sum u v, sum (u v)^2, sum |u v|) per row in numpy float64 from the float32 inputs"""
    U = U.double().cpu().numpy()
    sub = 0.0 if Pm is None else Pm.double().cpu().numpy() * rdiag.cpu().numpy()[:, None]
    u = U - sub
    v = u if V is None else V.double().cpu().numpy() - sub
    p = u * v
    return p.sum(1), (p * p).sum(1), np.abs(p).sum(1)


def _moments_err(acc, ref):
    """worst relative error of the two sums; the first is measured against sum |u v|, the size of its terms (it is a sum of
    signed products when U and V differ; the same number when they do not)"""
    a = acc.cpu().numpy()
    return max((np.abs(a[:, 0] - ref[0]) / ref[2]).max(), (np.abs(a[:, 1] - ref[1]) / ref[1]).max())


@pytest.mark.parametrize("C", [1, 3, 4, 64, 255, 256])
def test_row_moments_match_float64(mgp, dev, C):
    lib = mgp._lib.lib()
    n = 1556
    gen = torch.Generator(device="cpu").manual_seed(C)
    U, V, Pm = (torch.randn(n, C, generator=gen).to(dev) for _ in range(3))
    rdiag = (torch.rand(n, generator=gen, dtype=torch.float64) + 0.5).to(dev)
    cases = {"U, Pm": (U, None, rdiag, Pm), "U alone": (U, None, None, None), "U, V, Pm": (U, V, rdiag, Pm),
             "U, V": (U, V, None, None)}
    for name, (u, v, rd, pm) in cases.items():
        err = _moments_err(_moments(lib, u, v, rd, pm), _moments_ref(u, v, rd, pm))
        print("C = %d, %s: %.2e" % (C, name, err))
        assert err <= 1e-12, (name, err)
    # V == NULL is V == U
    assert torch.equal(_moments(lib, U, None, rdiag, Pm), _moments(lib, U, U, rdiag, Pm))
    # the state is read, added to and written back (the sums now carry the rounding of 2.5 + sum as well)
    acc = torch.full((n, 2), 2.5, dtype=torch.float64, device=dev)
    ref = _moments_ref(U, None, rdiag, Pm)
    got = _moments(lib, U, None, rdiag, Pm, acc=acc).cpu().numpy() - 2.5
    for k in (0, 1):
        assert (np.abs(got[:, k] - ref[k]) <= 1e-12 * (ref[k] + 2.5)).all(), k


def test_row_moments_chunks_alignment_and_argument_errors(mgp, dev):
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    n = 1556
    gen = torch.Generator(device="cpu").manual_seed(7)
    U, Pm = torch.randn(n, 32, generator=gen).to(dev), torch.randn(n, 32, generator=gen).to(dev)
    rdiag = (torch.rand(n, generator=gen, dtype=torch.float64) + 0.5).to(dev)
    # two chunks of 16 columns add up to the one call of 32
    acc = torch.zeros(n, 2, dtype=torch.float64, device=dev)
    for c0 in (0, 16):
        _moments(lib, U[:, c0:c0 + 16].contiguous(), None, rdiag, Pm[:, c0:c0 + 16].contiguous(), acc=acc)
    ref = _moments_ref(U, None, rdiag, Pm)
    assert _moments_err(acc, ref) <= 1e-12
    assert _moments_err(_moments(lib, U, None, rdiag, Pm), ref) <= 1e-12
    # rows that are not 16-byte aligned (a view one float into a buffer): the scalar loads
    flat = torch.randn(n * 4 + 1, generator=gen).to(dev)
    Uu = flat[1:].view(n, 4)
    assert Uu.data_ptr() % 16 == 4 and Uu.is_contiguous()
    P4 = Pm[:, :4].contiguous()
    assert _moments_err(_moments(lib, Uu, None, rdiag, P4), _moments_ref(Uu, None, rdiag, P4)) <= 1e-12
    assert _moments_err(_moments(lib, Uu.clone(), None, rdiag, P4), _moments_ref(Uu, None, rdiag, P4)) <= 1e-12   # aligned copy
    acc = torch.zeros(n, 2, dtype=torch.float64, device=dev)
    for C in (0, 257):
        assert lib.mgp_row_moments(_lib.ptr(U), None, None, None, n, C, _lib.ptr(acc), _lib.stream()) == -1
    assert not acc.any()


# ------------------------------------------------------------------------------------------------ the estimator
_DRAWS = {}       # Philox normals per fixture: they depend on (seed, S) and the edge list alone
_DENSE = {}


def _dense(g, case, norm, nu):
    key = (case, norm, nu)
    if key not in _DENSE:
        _DENSE.clear()
        _DENSE[key] = vref.Dense(g, norm, nu, SCALE)
    return _DENSE[key]


def _node_err(got, want):
    return float(np.abs(got.cpu().numpy() / want - 1.0).max())


@pytest.mark.parametrize("per_node", [False, True])
@pytest.mark.parametrize("nu", [2, 3])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("case", FIXTURES)
def test_posterior_variance_matches_float64_restatement(mgp, golden, dev, case, norm, nu, per_node):
    """Same seed, same Philox draws, dense float64 solves: var within 1e-4 relative at every node (the project's end-to-end
    posterior bar) at tol = 1e-6, refine = 1; se within 1e-3.  nu = 3 runs the edge stream."""
    from manifold_gp_amd import sampling
    g = golden(case)
    desc = _desc(mgp, g, dev, norm, nu)
    n, seed, S = desc.n, 11, 64
    noise, observed, var64, obs = _noise_case(n, dev, per_node)
    var, se = sampling.posterior_variance(desc, noise, S, seed, observed=observed)
    assert var.dtype == torch.float64 and se.dtype == torch.float64 and var.shape == (n,) and se.shape == (n,)
    assert var.device.type == "cuda"
    want_var, want_se = vref.reference(_dense(g, case, norm, nu), var64, obs, seed, S, cache=_DRAWS.setdefault(case, {}))
    ev, es = _node_err(var, want_var), _node_err(se, want_se)
    print("var: worst node %.2e; se: worst node %.2e; median se / var %.2e" % (ev, es, float((se / var).median())))
    assert ev <= 1e-4, ev
    assert es <= 1e-3, es
    assert bool((se > 0).all())


def test_chunks_of_256_samples(mgp, golden, dev):
    """S = 300 is two launches of the noise, the solve and the moments: against the restatement at S = 300 to the same bar,
    and S = 256 (the first chunk alone) against the restatement at S = 256.  The 44 samples of the second chunk, isolated as
    (300 var(300) - 256 var(256)) / 44, then carry at most the two calls' errors, 1e-4 (300 var(300) + 256 var(256)) / 44."""
    from manifold_gp_amd import sampling
    case, norm, nu = "dumbbell_k10_loop", "randomwalk", 2
    g = golden(case)
    desc = _desc(mgp, g, dev, norm, nu)
    noise, observed, var64, obs = _noise_case(desc.n, dev, True)
    dense, cache, seed = _dense(g, case, norm, nu), {}, 5
    delta, p, d, s = vref.draws(dense, var64, obs, seed, 300, cache)
    got, want = {}, {}
    for S in (300, 256):
        var, se = sampling.posterior_variance(desc, noise, S, seed, observed=observed)
        want_var, want_se = vref.estimate(delta[:, :S], p[:, :S], d, s)
        ev, es = _node_err(var, want_var), _node_err(se, want_se)
        print("S = %d: var %.2e se %.2e" % (S, ev, es))
        assert ev <= 1e-4 and es <= 1e-3, (S, ev, es)
        got[S], want[S] = var.cpu().numpy(), want_var
    tail = (300 * got[300] - 256 * got[256]) / 44
    want_tail = vref.estimate(delta[:, 256:], p[:, 256:], d, s)[0]
    bound = 1e-4 * (300 * want[300] + 256 * want[256]) / 44
    print("second chunk alone: worst node at %.2f of its bound" % (np.abs(tail - want_tail) / bound).max())
    assert (np.abs(tail - want_tail) <= bound).all()


def test_method_samples_is_the_mean_square_of_the_sampler(mgp, golden, dev):
    """method = "samples": mean over the draws of (posterior_samples - posterior_mean)^2 on the same seed, 1e-4 at every node."""
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k50_noloop")
    desc = _desc(mgp, g, dev, "symmetric", 2)
    y = T(g["train_y"], dev)
    S, seed = 64, 23
    for per_node in (False, True):
        noise, observed, _, _ = _noise_case(desc.n, dev, per_node)
        kw = dict(tol=1e-6, refine=1, observed=observed)
        var, se = sampling.posterior_variance(desc, noise, S, seed, method="samples", **kw)
        x = sampling.posterior_samples(desc, y, noise, S, seed, **kw).double()
        m = sampling.posterior_mean(desc, y, noise, **kw).double()
        want = ((x - m[None, :]) ** 2).mean(0)
        err = float((var / want - 1.0).abs().max())
        print("per-node noise %s: %.2e" % (per_node, err))
        assert err <= 1e-4, err
        rb = sampling.posterior_variance(desc, noise, S, seed, **kw)[0]
        assert not torch.equal(rb, var)


def test_noisy_adds_the_noise_variance(mgp, golden, dev):
    from manifold_gp_amd import sampling
    desc = _desc(mgp, golden("dumbbell_k10_loop"), dev, "randomwalk", 2)
    for per_node in (False, True):
        noise, observed, var64, _ = _noise_case(desc.n, dev, per_node)
        var, se = sampling.posterior_variance(desc, noise, 8, 3, observed=observed)
        nvar, nse = sampling.posterior_variance(desc, noise, 8, 3, observed=observed, noisy=True)
        assert torch.equal(nvar, var + T(var64, dev)) and torch.equal(nse, se)
        sd = sampling.posterior_stddev(desc, noise, 8, 3, observed=observed)
        assert torch.equal(sd, var.clamp_min(0).sqrt())


def test_nu_4_runs_plain_and_refuses_rao_blackwell(mgp, golden, dev):
    from manifold_gp_amd import sampling
    desc = _desc(mgp, golden("dumbbell_k50_noloop"), dev, "symmetric", 4)
    var, se = sampling.posterior_variance(desc, NOISE, 8, 1, method="samples")
    assert bool(torch.isfinite(var).all()) and bool((var > 0).all()) and bool((se > 0).all())
    with pytest.raises(NotImplementedError, match="samples"):
        sampling.posterior_variance(desc, NOISE, 8, 1)


def _model(mgp, g, dev, labeled=None):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    x, y = T(g["train_x"], dev), T(g["train_y"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=3, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    return RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev), labeled=labeled).to(dev)


def test_model_methods(mgp, golden, dev):
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    model = _model(mgp, g, dev)
    obs = T(np.random.default_rng(2).random(n) < 0.5, dev)
    desc = model.precision(noise=False)._descriptor()
    noise = float(model.likelihood.noise.detach().reshape(-1)[0])
    for kw in (dict(), dict(observed=obs), dict(observed=obs, noisy=True, method="samples")):
        var, se = model.precision_posterior_variance(16, seed=3, **kw)
        want_var, want_se = sampling.posterior_variance(desc, noise, 16, 3, **kw)
        assert torch.equal(var, want_var) and torch.equal(se, want_se)
        assert torch.equal(model.precision_posterior_stddev(16, seed=3, **kw), var.clamp_min(0).sqrt())
    semi = _model(mgp, g, dev, labeled=T(np.arange(n) < 100, dev))
    for fn in (semi.precision_posterior_variance, semi.precision_posterior_stddev):
        with pytest.raises(NotImplementedError):
            fn(4, seed=1)
