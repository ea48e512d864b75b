"""Eigensolver blocks of more than 256 columns (up to 512: num_modes up to 455 with the default block rule) on the GPU, through
the package classes, against float64.

Graph of tests 1, 3 and 4: tools.synth.dumbbell_resampled(4096) -- a closed curve, so the eigenvalues come in near-pairs and every m
here is odd: the cut keeps whole pairs --, symmetric normalisation, the library's own k-NN at k = 16, bandwidth TWICE the eps_min of
synth.bandwidth_rule (its `floor` argument).  At eps_min itself, which test_c2_dumbbell_10k_spmv_and_eigensolve takes, every weight
is <= 1e-4 and the fp32 Laplacian differs from the float64 one by the cancellation that test describes (4e-7 / eps^2): the control
below, run on the commit before wide blocks, then missed the eigenvalue bar by a factor 67 (m = 100 and 199 alike; orthonormality
0.003 and residuals 0.30 of their bars), so that graph is the wrong one for the purpose; at 2 eps_min and at 4 eps_min it meets
every bar, and 2 eps_min is the choice.  Reference: numpy.linalg.eigh in float64 of the dense oracle.sparse.laplacian_sym_csr
matrix, once per module.

Bars (the existing eigensolver tests' own): eigenvalues within 2e-6 max|diag L| of float64 (test_eigensolver_disconnected_components),
|V^T V - I| < 5e-5 (test_eigensolver_vs_dense_eigh_k50), reported residuals <= tol x Gershgorin bound with info[2] == m at tol = 1e-6.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K, TOL = 4096, 16, 1e-6
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


def _curve_graph(mgp, dev, n, k=K):
    """n points of the dumbbell curve -> k-NN graph, symmetric Laplacian at the bandwidth rule, the oracle's float64 matrix."""
    from oracle.laplacian import LaplacianOracle
    from oracle.sparse import laplacian_sym_csr
    from tools import synth
    x_np, y_np, _ = synth.dumbbell_resampled(n)
    x = T(x_np, dev)
    knn = mgp.utils.NearestNeighbors(x)
    D, _ = knn.search(x, k)
    idx, val = knn.graph(k)
    graph = knn.knn_graph
    eps_min = synth.bandwidth_rule(D[:, 1].cpu().numpy(), 0.0)[1]
    eps = synth.bandwidth_rule(D[:, 1].cpu().numpy(), 2.0 * eps_min)[0]          # 2 eps_min: see the module docstring
    op = mgp.operators.GraphLaplacianOperator(val, idx, n, torch.tensor([[eps]], device=dev), "symmetric", graph=graph)
    lo = LaplacianOracle(graph.edge_value.cpu().numpy(), graph.edge_index.cpu().numpy(), n, eps, "symmetric", True, dtype=np.float64)
    A = laplacian_sym_csr(lo).toarray()
    A = 0.5 * (A + A.T)
    return dict(x_np=x_np, y_np=y_np, x=x, eps=eps, op=op, lo=lo, A=A, maxdiag=float(np.abs(np.diag(A)).max()),
                gersh=float(np.abs(A).sum(1).max()))


@pytest.fixture(scope="module")
def curve(mgp, dev):
    g = _curve_graph(mgp, dev, N)
    g["w"], g["U"] = np.linalg.eigh(g["A"])          # float64, once
    return g


def _check_pairs(g, w, m, evals, evecs, resid, info, label):
    """The bars of the module docstring, the pairs ascending, and the backward error re-evaluated in float64 with the oracle's
    matrix: ||L v - theta v|| <= tol G + 2 dL, where dL = max(2e-6 lmax, 4e-7 / eps^2) bounds the difference between the fp32
    Laplacian the solver iterates on and the float64 one (test_c2_dumbbell_10k_spmv_and_eigensolve derives and uses it: entries
    of L are differences of O(1) terms over eps^2), once for the matrix and once for the fp32 product behind the solver's own
    residual.  The reported residuals are compared with the float64 Gershgorin bound widened by 1e-5 (the solver's bound is the
    fp32 row sum of 17 entries times 1 + 1e-6).  Returns the ratios to the bars."""
    ev = evals.double().cpu().numpy()
    V = evecs.double().cpu().numpy()
    assert V.shape == (g["A"].shape[0], m) and ev.shape == (m,)
    dL = max(2e-6 * 2.0 * g["maxdiag"], 4e-7 / g["eps"] ** 2)
    R = np.linalg.norm(g["A"] @ V - V * ev[None, :], axis=0)
    r = dict(evals=float(np.abs(ev - w[:m]).max() / (2e-6 * g["maxdiag"])),
             orth=float(np.abs(V.T @ V - np.eye(m)).max() / 5e-5),
             resid=float(max(resid) / (TOL * g["gersh"] * (1 + 1e-5))),
             backward=float(R.max() / (TOL * g["gersh"] * (1 + 1e-5) + 2 * dL)))
    print("%s: m %d block %d rounds %d products %d converged %d | ratios to the bars: %s" %
          (label, m, info[3], info[0], info[1], info[2], " ".join("%s %.3f" % kv for kv in r.items())))
    assert info[2] == m, info
    assert np.all(np.diff(ev) >= 0)
    assert r["evals"] <= 1.0 and r["orth"] < 1.0 and r["resid"] <= 1.0 and r["backward"] <= 1.0, r
    return r


def test_control_199_modes_one_launch_block(mgp, dev, curve):
    """The control: m = 199 is b = 256, the widest block of one SpMM launch, which ran before blocks went wider.  It must meet the
    bars on this graph, or the graph would be the wrong one for the wide cases.
    Measured (MI355X, the commit before wide blocks and this one: byte-identical evals and evecs), worst ratios to the bars:
    eigenvalues 0.007, orthonormality 0.003, reported residuals 0.950 (the solver's own stopping test), 4 rounds / 178 products."""
    from manifold_gp_amd.solvers import lanczos_smallest
    evals, evecs, resid = lanczos_smallest(curve["op"].data, 199, tol=TOL)
    info = list(lanczos_smallest.last_info)
    assert info[3] == 256
    _check_pairs(curve, curve["w"], 199, evals, evecs, resid, info, "control")


@pytest.mark.parametrize("m,b", [(229, 320), (299, 384), (447, 512)])
def test_wide_blocks_against_float64(mgp, dev, curve, m, b):
    """m = 229 (the first block past 256 columns: 320 = 160 + 160 per product), 299 (384 = 192 + 192), 447 (the cap: 512 = 256 +
    256): eigenvalues, orthonormality, reported residuals, ascending order and the float64 backward error at the bars.
    Measured (MI355X), ratios to the bars eigenvalues / orthonormality / reported residuals: m = 229 0.007 / 0.002 / 0.443 (4 rounds,
    276 products), 299 0.007 / 0.003 / 0.785 (4, 216), 447 0.007 / 0.002 / 0.799 (4, 212)."""
    from manifold_gp_amd.solvers import lanczos_smallest
    evals, evecs, resid = lanczos_smallest(curve["op"].data, m, tol=TOL)
    info = list(lanczos_smallest.last_info)
    assert info[3] == b
    _check_pairs(curve, curve["w"], m, evals, evecs, resid, info, "wide")


@pytest.mark.parametrize("n,m,b", [(300, 250, 300), (260, 229, 260)])
def test_block_equal_to_the_whole_space(mgp, dev, n, m, b):
    """b = min(320, n) = n columns: not a multiple of 64, chunks 152 + 148 (n = 300) and 132 + 128 (n = 260): the smallest shapes at
    which the chunking, the rotation at more than 256 modes and the workspace carving can go wrong.  Rayleigh-Ritz on the whole
    space is exact, so the bars are met within two rounds.
    Such a block is not filtered (eig_whole_space: the interval above its largest Ritz value holds no eigenvalue, and a polynomial
    that is small there lifts the lowest modes over mode m by more than float32 columns survive -- with the filter on, both shapes
    ran 60 rounds without one converged pair): rounds of degree 0, i.e. one launch per chunk and round.
    Measured (MI355X): both shapes 2 rounds / 4 launches; ratios to the bars eigenvalues / orthonormality / reported residuals
    0.134 / 0.004 / 0.267 (n = 300) and 0.061 / 0.003 / 0.281 (n = 260)."""
    from manifold_gp_amd.solvers import lanczos_smallest
    g = _curve_graph(mgp, dev, n)
    w = np.linalg.eigvalsh(g["A"])
    evals, evecs, resid = lanczos_smallest(g["op"].data, m, tol=TOL)
    info = list(lanczos_smallest.last_info)
    assert info[3] == b and info[0] <= 2, info
    _check_pairs(g, w, m, evals, evecs, resid, info, "whole space n = %d" % n)


def test_warm_start_and_block_outputs_at_384_columns(mgp, dev, curve):
    """m = 299, b = 384.  return_block hands out all 384 columns, and a float64 Rayleigh-Ritz of them with the oracle's matrix
    reproduces the first 299 eigenvalues at the eigenvalue bar; a second call warmed by the first returns the same eigenvalues
    within the bar in no more rounds."""
    from manifold_gp_amd.solvers import lanczos_smallest
    m, b = 299, 384
    A, w = curve["A"], curve["w"]
    bar = 2e-6 * curve["maxdiag"]
    ev1, V1, res1, blk = lanczos_smallest(curve["op"].data, m, tol=TOL, return_block=True, keep_warm=True)
    info1 = list(lanczos_smallest.last_info)
    warm = lanczos_smallest.last_warm
    assert blk["evecs"].shape == (N, b) and blk["evals"].shape == (b,) and len(blk["resid"]) == b and info1[3] == b
    assert torch.equal(blk["evecs"][:, :m], V1) and torch.equal(blk["evals"][:m], ev1)
    Vb = blk["evecs"].double().cpu().numpy()
    G, H = Vb.T @ Vb, Vb.T @ (A @ Vb)
    Lc = np.linalg.cholesky(0.5 * (G + G.T))
    Hp = np.linalg.solve(Lc, np.linalg.solve(Lc, 0.5 * (H + H.T)).T)
    th = np.linalg.eigvalsh(0.5 * (Hp + Hp.T))
    print("float64 Rayleigh-Ritz of the 384-column block: max |theta - lambda| / bar %.3f (first %d)" % (np.abs(th[:m] - w[:m]).max() / bar, m))
    assert np.abs(th[:m] - w[:m]).max() <= bar
    ev2, V2, res2 = lanczos_smallest(curve["op"].data, m, tol=TOL, warm=warm)
    info2 = list(lanczos_smallest.last_info)
    print("cold: rounds %d products %d; warm: rounds %d products %d" % (info1[0], info1[1], info2[0], info2[1]))
    assert info2[2] == m and info2[0] <= info1[0], (info1, info2)
    assert float((ev2 - ev1).abs().max()) <= bar
    assert np.abs(ev2.double().cpu().numpy() - w[:m]).max() <= bar


def test_downstream_of_eval_at_299_modes(mgp, dev, curve):
    """RiemannMaternKernel(num_modes = 299) -> eval() -> features (in-sample and at 64 held-out points of the curve) ->
    RiemannGP.posterior against the oracle's float64 pipeline fed the float64 eigenpairs (the layout of
    test_c2_dumbbell_10k_posterior_vs_dense_float64_pipeline): posterior mean and variance within the project's 1e-4 bar.
    kernel_block and kernel_diag at m = 299 against the float64 product of the same features at the fp32-rounding bound of
    test_kernel_block_two_half_walk_vs_one_tile_per_workgroup, 2e-6 max|K| sqrt(m / 16) + 1e-6; woodbury and exact_mll_lowrank
    take their Gram fast paths (m + 2 <= 512)."""
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.solvers import kernel_block, kernel_diag, woodbury
    from manifold_gp_amd.utils.train_model import exact_mll_lowrank
    from oracle import spectral as osp
    from oracle.solvers import gp_posterior_lowrank
    from tools import synth
    m, nu, s, noise = 299, 2, 0.7, 1e-2
    lo, w, U, eps = curve["lo"], curve["w"], curve["U"], curve["eps"]
    # Hyper-parameters at the scale of THIS graph (eps ~ 6e-4, eigenvalues up to ~1e5), not the unit-scale ones of the 10k test:
    # * length scale: 2 nu / kappa^2 = lambda_150, so that half of the 299 modes carry weight.  With kappa = 0.5 only the ~10
    #   modes under 2 nu / kappa^2 = 16 do, whose mutual gaps (~0.1 - 1) are below the eigensolver's tolerance tol x Gershgorin =
    #   0.86: that kernel is not a function of what the solver is asked to resolve (measured: kernel error 4.3e-4);
    # * bump decay (3 eps)^2: the bump's normaliser exp(-decay / (3 eps)^2) is then e^-1; with decay = 0.01 it is exp(-2857) = 0
    #   in float64 and the reference's own bump function returns 0 / 0.
    kappa = float(np.sqrt(2.0 * nu / w[m // 2]))
    bump = (3.0, float((3.0 * eps) ** 2))
    x, y_np = curve["x"], curve["y_np"]
    y = T(y_np, dev)
    xt_np = synth.dumbbell_resampled(2 * N)[0][1::2][np.random.default_rng(3).choice(N, 64, replace=False)]    # between the nodes
    xt = T(xt_np, dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=K, laplacian_normalization="symmetric", num_modes=m,
                                           bump_scale=bump[0], bump_decay=bump[1]).to(dev)
    kern.initialize(graphbandwidth=eps, lengthscale=kappa)
    model = RiemannGP(x, y, GaussianLikelihood(noise).to(dev), ScaleKernel(kern, s).to(dev)).to(dev)
    model.eval()
    model.posterior(xt)
    assert kern.eigvec.shape == (N, m) and kern.eigen_info[2] == m and kern.eigen_info[3] == 384, kern.eigen_info
    Dt, It = kern.knn.search(xt, K)
    lam = w[:m].copy()
    lam[0] = 0.0
    Phi = U[:, :m] * (lo.degree ** -0.5)[:, None]
    Phi /= np.linalg.norm(Phi, axis=0, keepdims=True)
    Z64 = osp.features_insample(lam, Phi, nu, kappa)
    Zt64 = osp.features_oos(lo, lam, Phi, nu, kappa, Dt.double().cpu().numpy(), It.cpu().numpy(), bump[0], bump[1])
    mean_o, cov_o, _ = gp_posterior_lowrank(Z64, y_np, Zt64, s, noise)
    mean, cov = model.posterior_mean.double().cpu().numpy(), model.posterior_covar.double().cpu().numpy()
    Zg, Ztg = kern.features(x), kern.features(xt)
    Z, Zt = Zg.double().cpu().numpy(), Ztg.double().cpu().numpy()
    e = dict(kernel=float(np.abs(Z[:256] @ Z.T - Z64[:256] @ Z64.T).max() / np.abs(Z64[:256] @ Z64.T).max()),
             cross=float(np.abs(Zt @ Z.T - Zt64 @ Z64.T).max() / np.abs(Zt64 @ Z64.T).max()),
             mean=float(np.abs(mean - mean_o).max() / np.abs(mean_o).max()),
             var=float(np.abs(np.diag(cov) - np.diag(cov_o)).max() / np.abs(np.diag(cov_o)).max()))
    print("m = 299 end to end vs the float64 pipeline: gap behind the kept block %.3e, eigensolver residual %.2e; %s"
          % (w[m] - w[m - 1], max(kern.eigen_residuals), " ".join("%s %.2e" % kv for kv in e.items())))
    assert (np.abs(Zt64).sum(1) > 0).mean() > 0.9                           # the held-out points lie in the bump support
    assert e["kernel"] < 1e-4 and e["cross"] < 1e-4 and e["mean"] < 1e-4 and e["var"] < 1e-4, e
    # ---- the dense block and its diagonal at 299 modes (the general kernel: the resident-operand one ends at 128)
    for A_, B_ in ((Zg[:517], Zg), (Ztg, Zg)):
        ref = A_.double() @ B_.double().t()
        bound = 2e-6 * float(ref.abs().max()) * (m / 16) ** 0.5 + 1e-6
        assert float((kernel_block(A_, B_).double() - ref).abs().max()) < bound
    dref = (Zg.double() * Zg.double()).sum(1)
    assert float((kernel_diag(Zg, Zg).double() - dref).abs().max()) < 2e-6 * float(dref.abs().max()) * (m / 16) ** 0.5 + 1e-6
    # ---- Woodbury: the Gram fast path (m + C <= 512, m C <= 6144) at C = 1 and 4, the library-GEMM fallback at C = 32
    for C in (1, 4, 32):
        Y = torch.stack([y * (1.0 + 0.1 * c) for c in range(C)], 1) if C > 1 else y
        wb = woodbury(Zg, Y, s, noise)
        Zd, Yd = Zg.double(), Y.double().reshape(N, -1)
        t = torch.linalg.solve(Zd.t() @ Zd + (noise / s) * torch.eye(m, device=dev, dtype=torch.float64), Zd.t() @ Yd)
        ref = ((Yd - Zd @ t) / noise).reshape(Y.shape)
        err = float((wb["alpha"].double() - ref).abs().max() / ref.abs().max())
        print("woodbury C = %d (%s): rel err %.2e" % (C, "Gram path" if m * C <= 6144 else "fallback", err))
        assert err < 1e-4, (C, err)
    loss = float(exact_mll_lowrank(model))
    Kd = s * (Z64 @ Z64.T) + noise * np.eye(N)
    Lk = np.linalg.cholesky(Kd)
    a = np.linalg.solve(Lk, y_np.astype(np.float64))
    ref_loss = 0.5 * (a @ a + 2.0 * np.log(np.diag(Lk)).sum() + N * np.log(2 * np.pi)) / N
    print("exact_mll_lowrank %.6f, float64 dense %.6f" % (loss, ref_loss))
    assert abs(loss - ref_loss) < 1e-4 * abs(ref_loss)


def test_more_modes_than_the_widest_block_is_a_value_error(mgp, dev, monkeypatch):
    """One mode past the cap raises ValueError that names the cap -- the largest m whose block, by mgp_lanczos_block_size, has at
    most 512 columns: 455 with the default rule -- and neither the workspace query nor a solve is called for it.  The cap itself is
    admitted (block of 512)."""
    from manifold_gp_amd import _lib, solvers
    from tools import synth
    lib = _lib.lib()
    cap = max(m for m in range(1, 513) if lib.mgp_lanczos_block_size(m, None) <= 512)
    assert cap == 455 and lib.mgp_lanczos_block_size(cap, None) == 512 and lib.mgp_lanczos_block_size(cap + 1, None) > 512
    n = 1024
    x = T(synth.dumbbell_resampled(n)[0], dev)
    knn = mgp.utils.NearestNeighbors(x)
    idx, val = knn.graph(8)
    op = mgp.operators.GraphLaplacianOperator(val, idx, n, torch.tensor([[0.05]], device=dev), "symmetric", graph=knn.knn_graph)
    assert solvers.max_num_modes(n) == cap
    called = []

    class Spy:
        def __getattr__(self, name):
            if name != "mgp_lanczos_block_size":
                called.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(solvers, "lib", lambda: Spy())
    with pytest.raises(ValueError, match=r"largest num_modes .* is %d\b" % cap):
        solvers.lanczos_smallest(op.data, cap + 1, tol=TOL)
    assert called == [], called
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=8, laplacian_normalization="symmetric", num_modes=cap + 1).to(dev)
    with pytest.raises(ValueError, match=r"is %d\b" % cap):
        kern.eval()
    assert not [c for c in called if c.startswith("mgp_lanczos")], called
    # a graph smaller than the widest block admits every m <= n: the block is the whole space
    assert solvers.max_num_modes(300) == 300
