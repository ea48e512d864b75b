"""Laplace fits on the spectral features, without a GPU (tests/_spectral_laplace_ref.py, manifold_gp_amd/spectral_laplace.py):
the weight-space restatement against the dense function-space Laplace approximation, an independent formula, for every family;
and the argument checks of the public functions, all of which are raised on the host before any device call."""
import numpy as np
import pytest
import torch

import _spectral_laplace_ref as sref

N, M, FRAC, S = 300, 20, 0.30, 2.0


def _problem(family, seed=5):
    rng = np.random.default_rng(seed)
    Z = sref.f32(rng.standard_normal((N, M)) / np.sqrt(M))
    ftrue = Z @ (np.sqrt(S) * rng.standard_normal(M))
    obs = rng.random(N) < FRAC
    mean = {"poisson": 0.5, "negative_binomial": 0.5}.get(family, 0.0)
    d, pub = sref.problem(family, ftrue, obs, seed + 1, mean=mean)
    return Z, d, pub


@pytest.mark.parametrize("family", sref.FAMILIES)
def test_weight_space_matches_function_space(family):
    """The two restatements iterate to a relative gradient of 1e-12; A >= I / s gives |w_1 - w_2|_2 <= s (|grad_1| + |grad_2|) with
    the rounding of the evaluated gradients on top; log Z within 1e-6 of |sum l| + w.w / (2 s) + |logdet|."""
    Z, d, _ = _problem(family)
    g0 = np.abs(sref.gradient(Z, d, S, np.zeros(M))).max()
    w, g, trace = sref.newton(Z, d, S, rtol=1e-12)
    dense = sref.dense_fit(Z, d, S, rtol=1e-12)
    rel_w, rel_d = np.abs(g).max() / g0, np.abs(dense["grad"]).max() / g0
    bound = sref.weight_bound(S, [g, dense["grad"]], [sref.gradient_rounding(Z, d, S, w)] * 2)
    diff = np.linalg.norm(w - dense["w"])
    lz, scale = sref.log_z(Z, d, S, w)
    print("%s: %d steps, relative gradients %.1e %.1e, |dw| %.2e (bound %.2e), log Z %.10g vs %.10g (%.1e of the scale)"
          % (family, len(trace), rel_w, rel_d, diff, bound, lz, dense["log_z"], abs(lz - dense["log_z"]) / scale))
    assert rel_w <= 1e-12 and rel_d <= 1e-12
    assert diff <= bound
    assert abs(lz - dense["log_z"]) <= 1e-6 * max(scale, dense["scale"])
    # the latent variance of the weight space against the function space's: z*^T A^-1 z* = k** - k*^T (K + W^-1)^-1 k* on the
    # observed rows, here through B: s z*.z* - s^2 z*^T Z_o^T W^1/2 B^-1 W^1/2 Z_o z*
    Zo = Z[d["obs"]]
    h = sref.site(sref._restrict(d), dense["f"])[2]
    sw = np.sqrt(h)
    B = np.eye(Zo.shape[0]) + sw[:, None] * (S * Zo @ Zo.T) * sw[None, :]
    zs = Z[:7]
    c = sw[:, None] * (S * Zo @ zs.T)
    var_dense = S * np.einsum("ij,ij->i", zs, zs) - np.einsum("ij,ij->j", c, np.linalg.solve(B, c))
    _, var = sref.latent(zs, d, S, Z, w)
    assert np.abs(var - var_dense).max() <= 1e-9 * S * np.einsum("ij,ij->i", zs, zs).max()


# ------------------------------------------------------------------------------------------------ the host-side checks
def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def _fit_args(family):
    Z, d, pub = _problem(family)
    kw = {k: (v if np.isscalar(v) else _t(v, torch.float64)) for k, v in pub.items() if v is not None and k != "y"}
    if "num_categories" in kw:
        kw["num_categories"] = int(pub["num_categories"])
    return _t(Z), _t(pub["y"]), _t(d["obs"], torch.bool), kw


def test_fit_refuses_bad_arguments_on_the_host():
    from manifold_gp_amd.spectral_laplace import spectral_laplace_fit as fit
    Z, y, obs, kw = _fit_args("bernoulli")
    with pytest.raises(ValueError, match=r"float tensor \[n, m\]"):
        fit(Z.reshape(-1), y, obs)
    with pytest.raises(ValueError, match="1 .. 512 modes"):
        fit(torch.zeros(8, 513), y[:8], None)
    with pytest.raises(ValueError, match="y must be a tensor of %d labels" % N):
        fit(Z, y[:-1], obs)
    with pytest.raises(ValueError, match="observed has shape"):
        fit(Z, y, obs[:-1])
    with pytest.raises(ValueError, match="observed must be a bool tensor"):
        fit(Z, y, obs.float())
    with pytest.raises(ValueError, match="observed selects no node"):
        fit(Z, y, torch.zeros(N, dtype=torch.bool))
    bad = y.clone()
    bad[int(obs.nonzero()[0])] = 2.0
    with pytest.raises(ValueError, match="must all be 0 or 1"):
        fit(Z, bad, obs)
    with pytest.raises(ValueError, match="family must be one of"):
        fit(Z, y, obs, family="softmax")
    with pytest.raises(ValueError, match="outputscale must be finite and positive"):
        fit(Z, y, obs, outputscale=0.0)
    with pytest.raises(ValueError, match="mean must be finite"):
        fit(Z, y, obs, mean=float("nan"))
    with pytest.raises(ValueError, match="w0 must be a float tensor of %d weights" % M):
        fit(Z, y, obs, w0=torch.zeros(M + 1))
    with pytest.raises(ValueError, match="belong to the count families"):
        fit(Z, y, obs, trials=y)
    with pytest.raises(ValueError, match="belong to the ordinal family"):
        fit(Z, y, obs, num_categories=3)


def test_count_fits_refuse_bad_arguments_on_the_host():
    from manifold_gp_amd.spectral_laplace import spectral_laplace_fit as fit
    Z, y, obs, kw = _fit_args("binomial")
    first = int(obs.nonzero()[0])
    low = kw["trials"].clone()
    low[first] = y[first].double() - 1.0 if y[first] >= 2 else 0.0
    with pytest.raises(ValueError, match="trials"):
        fit(Z, y, obs, family="binomial", trials=low)
    small = kw["trials"].clone()
    y2 = y.clone()
    y2[first], small[first] = 5.0, 3.0
    with pytest.raises(ValueError, match="trials must be at least the counts"):
        fit(Z, y2, obs, family="binomial", trials=small)
    with pytest.raises(ValueError, match="the binomial family needs trials"):
        fit(Z, y, obs, family="binomial")
    Z, y, obs, kw = _fit_args("negative_binomial")
    for r in (2.0 ** -11, 2.0 ** 21, float("nan")):
        with pytest.raises(ValueError, match=r"dispersion must be a finite scalar in \[2\^-10, 2\^20\]"):
            fit(Z, y, obs, family="negative_binomial", exposure=kw["exposure"], dispersion=r)
    with pytest.raises(ValueError, match="needs dispersion="):
        fit(Z, y, obs, family="negative_binomial", exposure=kw["exposure"])
    half = y.clone()
    half[first] = 0.5
    with pytest.raises(ValueError, match=r"integers in \[0, 2\^24\]"):
        fit(Z, half, obs, family="poisson")
    with pytest.raises(ValueError, match="exposure at the observed nodes must be finite and positive"):
        fit(Z, y, obs, family="poisson", exposure=-kw["exposure"])


def test_ordinal_fit_refuses_bad_arguments_on_the_host():
    from manifold_gp_amd.spectral_laplace import spectral_laplace_fit as fit
    Z, y, obs, kw = _fit_args("ordinal")
    with pytest.raises(ValueError, match="needs num_categories"):
        fit(Z, y, obs, family="ordinal")
    with pytest.raises(ValueError, match="cutpoints must be strictly increasing"):
        fit(Z, y, obs, family="ordinal", num_categories=4, cutpoints=torch.tensor([0.0, -1.0, 1.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="cutpoints must be a real tensor of 3 values"):
        fit(Z, y, obs, family="ordinal", num_categories=4, cutpoints=torch.tensor([0.0, 1.0], dtype=torch.float64))
    with pytest.raises(ValueError, match=r"integers in \[0, 3\)"):
        fit(Z, y, obs, family="ordinal", num_categories=3)


@pytest.mark.parametrize("family", sref.FAMILIES)
def test_fit_refuses_host_tensors(family):
    """valid arguments on the host pass every check and are refused as host tensors: there is no CPU path"""
    from manifold_gp_amd.spectral_laplace import spectral_laplace_fit as fit
    Z, y, obs, kw = _fit_args(family)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit(Z, y, obs, family=family, **kw)


def test_site_wrapper_refuses_bad_arguments_on_the_host():
    from manifold_gp_amd.spectral_laplace import spectral_site
    Z, y, obs, _ = _fit_args("bernoulli")
    w = torch.zeros(M, dtype=torch.float64)
    with pytest.raises(ValueError, match="1 .. 512 modes"):
        spectral_site(torch.zeros(4, 600), torch.zeros(600), "bernoulli", torch.zeros(4))
    with pytest.raises(ValueError, match="w must be a float tensor of %d weights" % M):
        spectral_site(Z, w[:-1], "bernoulli", y)
    with pytest.raises(ValueError, match="a must be a tensor of %d values" % N):
        spectral_site(Z, w, "bernoulli", y[:-1])
    with pytest.raises(ValueError, match="needs the trials in b"):
        spectral_site(Z, w, "binomial", y)
    with pytest.raises(ValueError, match="needs the upper cutpoints in b"):
        spectral_site(Z, w, "ordinal", y)
    with pytest.raises(ValueError, match="needs dispersion="):
        spectral_site(Z, w, "negative_binomial", y)
    with pytest.raises(ValueError, match="dispersion belongs to the negative_binomial family"):
        spectral_site(Z, w, "poisson", y, dispersion=1.0)
    with pytest.raises(ValueError, match="observed must be a bool tensor"):
        spectral_site(Z, w, "bernoulli", y, observed=obs[:-1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        spectral_site(Z, w, "bernoulli", y, observed=obs)


def test_fit_object_refuses_what_its_family_lacks():
    from manifold_gp_amd.spectral_laplace import SpectralLaplaceFit
    w = torch.zeros(3, dtype=torch.float64)
    fit = SpectralLaplaceFit(w, torch.eye(3, dtype=torch.float64) / 2.0 ** 0.5, torch.zeros(5, dtype=torch.float64), True, 0, [], -1.0,
                             "poisson", 2.0, 0.0)
    with pytest.raises(NotImplementedError, match="class probability"):
        fit.predict_proba(torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r"\[T, 3\] feature rows"):
        fit.latent(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.latent(torch.zeros(2, 3))
    # log Z of the prior alone: A = I / s, logdet(s A) = 0
    assert abs(fit.log_evidence() + 1.0) <= 1e-15
