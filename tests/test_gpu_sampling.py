"""Exact GMRF sampling on the MI355X (manifold_gp_amd/sampling.py, csrc/sampling.hip): the noise kernel against its numpy
restatement, determinism and chunk invariance, prior / posterior samples against a dense float64 oracle fed the same
noise, sample statistics against the exact covariances, the public methods, and the perturbed system at C3's size."""
import math

import numpy as np
import pytest
import torch

from _sampling_ref import edge_factor, edge_noise, gmrf_noise_ref, node_noise

pytestmark = pytest.mark.gpu

CASES = ["dumbbell_k10_loop", "dumbbell_k50_noloop"]
NORMS = ["symmetric", "randomwalk"]
SEEDS = [1, 0x0123456789ABCDEF]


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


def _lap(mgp, g, dev, norm):
    idx = T(g["edge_index"].astype(np.int64), dev)
    val = T(g["edge_value"], dev)
    eps = torch.tensor([[float(g["eps"])]], device=dev)
    return mgp.operators.GraphLaplacianOperator(val, idx, g["train_x"].shape[0], eps, norm, bool(g["self_loops"]))


def _csr_host(data):
    gr = data.graph
    return (gr.rowptr.cpu().numpy(), gr.col.cpu().numpy(), data.vals.double().cpu().numpy(), data.dsqrt.double().cpu().numpy())


# ------------------------------------------------------------------------------------------------ the noise kernel
@pytest.mark.parametrize("case", CASES)
def test_noise_kernel_vs_numpy_restatement(mgp, golden, dev, case):
    from manifold_gp_amd.sampling import gmrf_noise
    g = golden(case)
    data = _lap(mgp, g, dev, "randomwalk").data
    rowptr, col, vals, dsqrt = _csr_host(data)
    coef = 1.7
    for S, offset in [(1, 0), (3, 0), (4, 0), (17, 0), (64, 0), (17, 5), (3, 258)]:
        for seed in SEEDS:
            for tag in (0, 2):
                for edges in (False, True):
                    Y = gmrf_noise(data, S, seed, offset, node_coef=coef, tag=tag, edges=edges).double().cpu().numpy()
                    ref, l1 = gmrf_noise_ref(rowptr, col, vals, dsqrt, coef, tag, edges, seed, offset, S)
                    err = np.abs(Y - ref).max()
                    assert err <= 1e-5 * l1, (S, offset, seed, tag, edges, err, l1)


def test_noise_kernel_deterministic_and_chunk_invariant(mgp, golden, dev):
    from manifold_gp_amd.sampling import gmrf_noise
    data = _lap(mgp, golden("dumbbell_k50_noloop"), dev, "symmetric").data
    for S in (3, 64, 300):
        a = gmrf_noise(data, S, 99, node_coef=0.3, edges=True)
        b = gmrf_noise(data, S, 99, node_coef=0.3, edges=True)
        assert torch.equal(a, b), S
    full = gmrf_noise(data, 64, 5, 0, node_coef=0.8, edges=True)
    part = gmrf_noise(data, 16, 5, 16, node_coef=0.8, edges=True)
    assert torch.equal(full[:, 16:32], part)
    big = gmrf_noise(data, 300, 5, 0, node_coef=0.8, tag=2, edges=True)
    assert torch.equal(big[:, :256], gmrf_noise(data, 256, 5, 0, node_coef=0.8, tag=2, edges=True))
    assert torch.equal(big[:, 256:], gmrf_noise(data, 44, 5, 256, node_coef=0.8, tag=2, edges=True))
    # streams and seeds differ
    assert not torch.equal(gmrf_noise(data, 8, 5, tag=0), gmrf_noise(data, 8, 5, tag=2))
    assert not torch.equal(gmrf_noise(data, 8, 5), gmrf_noise(data, 8, 6))


# ------------------------------------------------------------------------------------------------ samples vs dense float64
def _dense(g, norm, nu, kappa, scale):
    from oracle.laplacian import LaplacianOracle
    from oracle.precision import dense_matern_precision
    lo = LaplacianOracle(g["edge_value"], g["edge_index"], g["train_x"].shape[0], float(g["eps"]), norm,
                         bool(g["self_loops"]), dtype=np.float64)
    n = lo.n
    tau = 2.0 * nu / kappa ** 2
    A = tau * np.eye(n) + lo.dense_symmetric()
    P = np.sqrt(lo.degree) if norm == "randomwalk" else np.ones(n)
    Q2 = scale * dense_matern_precision(lo.dense(), nu, kappa, lo.degree if norm == "randomwalk" else None)
    r, c = lo.idx[0], lo.idx[1]
    E = edge_factor(n, r, c, lo.triu, np.sqrt(lo.degree))
    return dict(n=n, tau=tau, A=A, P=P, Q2=Q2, r=r, c=c, E=E)


def _base_noise_ref(d, nu, seed, S):
    """g = sqrt(tau) w + E w_edge (odd nu) or w (even nu), and k of z = sqrt(scale) P A^k noise."""
    w = node_noise(d["n"], 0, seed, 0, S)
    if nu % 2:
        return math.sqrt(d["tau"]) * w + d["E"] @ edge_noise(d["r"], d["c"], seed, 0, S), (nu - 1) // 2
    return w, nu // 2


def _colerr(x, ref):
    return float((np.abs(x - ref).max(axis=0) / np.abs(ref).max(axis=0)).max())


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("nu", [1, 2, 3])
def test_prior_posterior_precision_vs_dense_fp64(mgp, golden, dev, norm, nu):
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k10_loop")
    kappa, scale, s, S, seed = float(g["kappa"]), 0.7, 1e-2, 6, 4242
    lap = _lap(mgp, g, dev, norm)
    desc = mgp.operators.PrecisionMaternOperator(lap, nu, torch.tensor([[kappa]], device=dev))._descriptor().with_(scale=scale)
    d = _dense(g, norm, nu, kappa, scale)
    noise, k = _base_noise_ref(d, nu, seed, S)
    P = d["P"][:, None]
    z_ref = math.sqrt(scale) * P * (np.linalg.matrix_power(d["A"], k) @ noise)
    kf = (nu + 1) // 2 if nu % 2 else nu // 2
    f_ref = P ** -1 / math.sqrt(scale) * np.linalg.solve(np.linalg.matrix_power(d["A"], kf), noise)
    y = g["train_y"].astype(np.float64)
    w2 = node_noise(d["n"], 2, seed, 0, S)
    x_ref = np.linalg.solve(np.eye(d["n"]) + s * d["Q2"], y[:, None] + s * z_ref + math.sqrt(s) * w2)
    z = sampling.precision_samples(desc, S, seed).double().cpu().numpy().T
    f = sampling.prior_samples(desc, S, seed, tol=1e-6, refine=3).double().cpu().numpy().T
    x = sampling.posterior_samples(desc, T(g["train_y"], dev), s, S, seed, tol=1e-6, refine=3).double().cpu().numpy().T
    assert _colerr(z, z_ref) < 1e-4, _colerr(z, z_ref)
    assert _colerr(f, f_ref) < 1e-4, _colerr(f, f_ref)
    assert _colerr(x, x_ref) < 1e-4, _colerr(x, x_ref)
    # noisy: + sqrt(s) w3 on the same latent sample
    xn = sampling.posterior_samples(desc, T(g["train_y"], dev), s, S, seed, noisy=True, tol=1e-6, refine=3).double().cpu().numpy().T
    assert _colerr(xn, x_ref + math.sqrt(s) * node_noise(d["n"], 3, seed, 0, S)) < 1e-4


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("norm,nu", [("randomwalk", 2), ("symmetric", 3)])
def test_sample_statistics_match_exact_covariances(mgp, golden, dev, norm, nu):
    from manifold_gp_amd import sampling
    g = golden("dumbbell_k10_loop")
    kappa, scale, s, S = float(g["kappa"]), 1.3, 5e-2, 2048
    lap = _lap(mgp, g, dev, norm)
    desc = mgp.operators.PrecisionMaternOperator(lap, nu, torch.tensor([[kappa]], device=dev))._descriptor().with_(scale=scale)
    d = _dense(g, norm, nu, kappa, scale)
    V = np.random.default_rng(8).standard_normal((d["n"], 8))
    bound = 6.0 * math.sqrt(2.0 / S)
    f = sampling.prior_samples(desc, S, 17).double().cpu().numpy()
    cov = np.linalg.inv(d["Q2"])
    want = np.einsum("ip,ij,jp->p", V, cov, V)
    got = ((f @ V) ** 2).mean(0)
    assert (np.abs(got / want - 1.0) < bound).all(), (got / want)
    y = T(g["train_y"], dev)
    x = sampling.posterior_samples(desc, y, s, S, 18).double().cpu().numpy()
    cov = np.linalg.inv(d["Q2"] + np.eye(d["n"]) / s)
    mean = sampling.posterior_mean(desc, y, s).double().cpu().numpy()
    dev_ = (x - mean[None, :]) @ V
    want = np.einsum("ip,ij,jp->p", V, cov, V)
    got = (dev_ ** 2).mean(0)
    assert (np.abs(got / want - 1.0) < bound).all(), (got / want)
    assert (np.abs(dev_.mean(0)) < 6.0 * np.sqrt(want / S)).all()


# ------------------------------------------------------------------------------------------------ public methods
def _model(mgp, g, dev, nu=3, labeled=None):
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    x, y = T(g["train_x"], dev), T(g["train_y"], dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=int(g["k"]), laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=float(g["eps"]), lengthscale=float(g["kappa"]))
    return RiemannGP(x, y, GaussianLikelihood(2e-2).to(dev), ScaleKernel(kern, 0.8).to(dev), labeled=labeled).to(dev)


def test_public_sampling_api(mgp, golden, dev):
    g = golden("dumbbell_k10_loop")
    n = g["train_x"].shape[0]
    model = _model(mgp, g, dev)
    for out in (model.sample_prior(5, seed=3), model.sample_posterior(5, seed=3), model.sample_posterior(5, seed=3, noisy=True),
                model.precision(noise=False).zero_mean_mvn_samples(5, seed=3),
                model.base_kernel.precision().zero_mean_mvn_samples(5, seed=3)):
        assert out.shape == (5, n) and out.dtype == torch.float32 and out.device.type == "cuda"
        assert torch.isfinite(out).all()
    mean = model.precision_posterior_mean()
    assert mean.shape == (n,) and mean.dtype == torch.float32
    # seed=None draws from torch's default CPU generator
    torch.manual_seed(7)
    a = model.sample_posterior(3)
    torch.manual_seed(7)
    assert torch.equal(a, model.sample_posterior(3))
    assert not torch.equal(a, model.sample_posterior(3))
    from manifold_gp_amd.sampling import draw_seed
    torch.manual_seed(7)
    drawn = draw_seed()
    torch.manual_seed(7)
    assert torch.equal(model.sample_prior(2), model.sample_prior(2, seed=drawn))
    # the scale rides in the wrapper: N(0, s Q) = sqrt(s) N(0, Q) on the same noise
    zs = model.precision(noise=False).zero_mean_mvn_samples(4, seed=11)
    zq = model.base_kernel.precision().zero_mean_mvn_samples(4, seed=11)
    assert torch.allclose(zs, zq * math.sqrt(0.8), rtol=1e-5, atol=1e-6 * float(zq.abs().max()))
    semi = _model(mgp, g, dev, labeled=T(np.arange(n) < 100, dev))
    for fn in (lambda: semi.sample_prior(2, seed=1), lambda: semi.sample_posterior(2, seed=1), lambda: semi.precision_posterior_mean()):
        with pytest.raises(NotImplementedError):
            fn()


# ------------------------------------------------------------------------------------------------ C3 size
def test_c3_manifold784_posterior_samples(mgp, dev):
    """60k manifold_784 graph (k = 50, random walk, nu = 2), S = 16: the true residual of the perturbed system, recomputed in
    float64 from the same z, meets tol; the mean of ||z_j||^2 is within 6 standard deviations of tr(Q2)."""
    import scipy.sparse as sp
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
    xs = model.sample_posterior(S, seed=seed, tol=tol).double().cpu().numpy().T
    desc = model.precision(noise=False)._descriptor()
    rhs = sampling.posterior_rhs(desc, y, noise, S, seed).double().cpu().numpy()
    z = sampling.precision_samples(desc, S, seed).double().cpu().numpy().T
    # float64 operator from the device CSR: A = tau I + L_sym, Q2 = scale P A^2 P
    data = desc.data
    gr = data.graph
    rowptr, col = gr.rowptr.cpu().numpy(), gr.col.cpu().numpy()
    L = sp.csr_matrix((-data.vals.double().cpu().numpy(), col, rowptr), shape=(n, n)) + sp.diags(data.diag.double().cpu().numpy())
    A = (2.0 * nu / desc.kappa ** 2) * sp.identity(n) + L
    P = sp.diags(data.dsqrt.double().cpu().numpy())
    AP = (A @ P).tocsr()
    Q2 = desc.scale * (AP.T @ AP)
    r = rhs - (xs + noise * (Q2 @ xs))
    rel = np.linalg.norm(r, axis=0) / np.linalg.norm(rhs, axis=0)
    assert rel.max() <= tol, rel
    # the right-hand side is y + s z + sqrt(s) w2 with this z
    w2 = rhs - y_np.astype(np.float64)[:, None] - noise * z
    assert abs(w2.var() / noise - 1.0) < 0.05
    tr = float(Q2.diagonal().sum())
    sd = math.sqrt(2.0 * float(Q2.multiply(Q2).sum()) / S)
    m2 = float((z ** 2).sum(0).mean())
    assert abs(m2 - tr) < 6.0 * sd, (m2, tr, sd)
