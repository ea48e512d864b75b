"""RiemannGP on MI355X -- the model class of manifold_gp/models/riemann_gp.py:10-75.

Same constructor, `precision`, `modulation`, `posterior`, `posterior_mean / covar / stddev` and
`base_kernel` as the reference.  The reference inherits the posterior from gpytorch.models.ExactGP
(prediction strategy for a LowRankRootAddedDiagLinearOperator = Woodbury on the m x m root, SURVEY.md
Appendix B); gpytorch is not in this image, so the same algebra is spelled out here on device:

    K = s Z Z^T,  C = (n/s) I + Z^T Z                       (m x m, fp64, Cholesky)
    (K + n I)^-1 v = (v - Z C^-1 Z^T v) / n
    mean(x*)  = c + s Z* Z^T (K + n I)^-1 (y - c)
    cov(x*)   = s Z* [I - (s/n)(G - G C^-1 G)] Z*^T,  G = Z^T Z      (kernel block on the fp32 MFMA)

with Z = kernel.features(train_x), Z* = kernel.features(x*) (fused out-of-sample HIP kernel), s the
output scale, n the noise.  The hybrid posterior (riemann_gp.py:45-75) blends a Euclidean base model
with weight 1 - bump(distance to the nearest training point).
"""
import torch

from .. import _lib
from .._compat import HAVE_GPYTORCH, Positive
from ..operators import NoiseWrapperOperator, ScaleWrapperOperator, SchurComplementOperator
from ..utils import bump_function


class GaussianLikelihood(torch.nn.Module):
    """The one attribute of gpytorch.likelihoods.GaussianLikelihood the path reads: `noise`."""

    def __init__(self, noise=1e-2):
        super().__init__()
        self._constraint = Positive()
        self.raw_noise = torch.nn.Parameter(self._constraint.inverse_transform(torch.tensor([float(noise)])))

    @property
    def noise(self):
        return self._constraint.transform(self.raw_noise)

    @noise.setter
    def noise(self, value):
        with torch.no_grad():
            self.raw_noise.copy_(self._constraint.inverse_transform(torch.as_tensor([float(value)]).to(self.raw_noise)))


class ScaleKernel(torch.nn.Module):
    """gpytorch.kernels.ScaleKernel as far as RiemannGP uses it: `base_kernel`, `outputscale`."""

    def __init__(self, base_kernel, outputscale=1.0):
        super().__init__()
        self.base_kernel = base_kernel
        self._constraint = Positive()
        self.raw_outputscale = torch.nn.Parameter(self._constraint.inverse_transform(torch.tensor(float(outputscale))))

    @property
    def outputscale(self):
        return self._constraint.transform(self.raw_outputscale)

    @outputscale.setter
    def outputscale(self, value):
        with torch.no_grad():
            self.raw_outputscale.copy_(self._constraint.inverse_transform(torch.as_tensor(float(value)).to(self.raw_outputscale)))

    def features(self, x):
        return self.base_kernel.features(x) * self.outputscale.sqrt().to(x.device)


class _Posterior:
    """mean / covariance / stddev of a Gaussian posterior at the test inputs."""

    def __init__(self, mean, covar):
        self.mean, self.covariance_matrix = mean, covar

    @property
    def stddev(self):
        return self.covariance_matrix.diagonal().clamp_min(0).sqrt()


class RiemannGP(torch.nn.Module):
    def __init__(self, train_x, train_y, likelihood, kernel, labeled=None):
        super().__init__()
        _lib.require_device(train_x, train_y)
        self.train_inputs = (train_x,)
        self.train_targets = train_y
        self.likelihood = likelihood
        self.covar_module = kernel
        self.labeled = labeled
        self.mean_constant = torch.nn.Parameter(torch.zeros(()))     # gpytorch.means.ConstantMean
        self._cache = None

    # ------------------------------------------------------------------ riemann_gp.py:23-39
    def eval(self):
        self.base_kernel.eval()
        self._cache = None
        return super().eval()

    @property
    def base_kernel(self):
        return self.covar_module.base_kernel if hasattr(self.covar_module, "base_kernel") else self.covar_module

    def precision(self, noise=True):
        opt = self.base_kernel.precision()
        if self.labeled is not None:
            opt = SchurComplementOperator(opt, self.labeled)
        if hasattr(self.covar_module, "outputscale"):
            opt = ScaleWrapperOperator(opt, self.covar_module.outputscale)
        if noise:
            opt = NoiseWrapperOperator(opt, self.likelihood.noise)
        return opt

    # ------------------------------------------------------------------ exact samples at the graph nodes (precision form)
    def _sampling_args(self):
        """(descriptor of precision(noise=False), likelihood noise, train_targets); semi-supervised models are not sampled."""
        if self.labeled is not None:
            raise NotImplementedError("sampling of semi-supervised (Schur-complement) models is not supported")
        desc = getattr(self.precision(noise=False), "_descriptor", lambda: None)()
        return desc, self._scale_noise()[1], self.train_targets

    def sample_prior(self, num_samples, seed=None, tol=1e-5):
        """f ~ N(0, Q^-1) at every graph node: [num_samples, N] float32 (sampling.prior_samples)."""
        from ..sampling import prior_samples
        desc, _, _ = self._sampling_args()
        return prior_samples(desc, num_samples, seed, tol=tol)

    def sample_posterior(self, num_samples, seed=None, noisy=False, tol=1e-5, observed=None):
        """f | y at every graph node by perturb-and-MAP: [num_samples, N] float32 with mean precision_posterior_mean() and
        covariance (Q + I / noise)^-1; noisy=True adds the likelihood noise (sampling.posterior_samples).  observed (bool [N]):
        condition on train_targets[observed] only -- the transductive posterior at the other nodes (operator form 3)."""
        from ..sampling import posterior_samples
        desc, noise, y = self._sampling_args()
        return posterior_samples(desc, y, noise, num_samples, seed, noisy=noisy, tol=tol, observed=observed)

    def precision_posterior_mean(self, tol=1e-5, observed=None):
        """(I + noise Q)^-1 y at every graph node: [N] float32 (sampling.posterior_mean).  observed (bool [N]): the mean
        conditioned on train_targets[observed] only, at every node."""
        from ..sampling import posterior_mean
        desc, noise, y = self._sampling_args()
        return posterior_mean(desc, y, noise, tol=tol, observed=observed)

    def precision_posterior_variance(self, num_samples=64, seed=None, observed=None, noisy=False, tol=1e-6,
                                     method="rao-blackwell"):
        """(var, se): the marginal variance of f | y at every graph node, diag((Q + W / noise)^-1), and the standard error of
        the estimate: float64 [N] each, from num_samples perturb-and-MAP draws (sampling.posterior_variance: single-site
        Rao-Blackwell for nu <= 3, method="samples" for the plain mean of squares).  observed as in sample_posterior;
        noisy=True adds the likelihood noise."""
        from ..sampling import posterior_variance
        desc, noise, _ = self._sampling_args()
        return posterior_variance(desc, noise, num_samples, seed, observed=observed, method=method, noisy=noisy, tol=tol)

    def precision_posterior_stddev(self, num_samples=64, seed=None, observed=None, noisy=False, tol=1e-6,
                                   method="rao-blackwell"):
        """sqrt of precision_posterior_variance(...)[0]: float64 [N]."""
        return self.precision_posterior_variance(num_samples, seed, observed, noisy, tol, method)[0].clamp_min(0).sqrt()

    def laplace_posterior(self, observed=None, **kw):
        """Classify the graph nodes: train_targets are 0/1 labels, read at `observed` (bool [N]; None: every node; NaN allowed
        elsewhere).  The Laplace approximation of the latent posterior under a Bernoulli-logit likelihood, a
        classification.LaplaceFit (mode, latent variances and samples, class probabilities); kw as classification.laplace_fit.
        The Gaussian likelihood's noise is not used."""
        from ..classification import laplace_fit
        desc, _, y = self._sampling_args()
        return laplace_fit(desc, y, observed, **kw)

    def laplace_posterior_multiclass(self, num_classes, observed=None, **kw):
        """Classify the graph nodes into num_classes classes: train_targets are class indices in [0, num_classes), read at
        `observed` (bool [N]; None: every node; NaN allowed elsewhere).  The Laplace approximation of the latent posterior
        under a softmax likelihood, a classification.MulticlassLaplaceFit (mode, latent samples, class probabilities); kw as
        classification.laplace_fit_multiclass.  The Gaussian likelihood's noise is not used.  The fit's latent_samples,
        predict_proba and latent_variance take block=b to draw b samples per solve (b num_classes <= 256)."""
        from ..classification import laplace_fit_multiclass
        desc, _, y = self._sampling_args()
        return laplace_fit_multiclass(desc, y, num_classes, observed, **kw)

    def laplace_posterior_counts(self, observed=None, **kw):
        """Counts at the graph nodes: train_targets are counts, read at `observed` (bool [N]; None: every node; NaN allowed
        elsewhere).  The Laplace approximation of the latent posterior under a Poisson (with exposure=), a binomial (with
        trials=) or a negative-binomial (family="negative_binomial" with dispersion= and exposure=) likelihood, a
        counts.CountLaplaceFit (mode, latent variances and samples, predicted counts); kw as counts.laplace_fit_counts (family,
        dispersion, exposure, trials, mean, step_tol, ...).  The Gaussian likelihood's noise is not
        used."""
        from ..counts import fit_counts
        desc, _, y = self._sampling_args()
        return fit_counts(desc, y, observed, **kw)

    def laplace_posterior_ordinal(self, num_categories, cutpoints=None, observed=None, **kw):
        """Ordered categories at the graph nodes: train_targets are categories in [0, num_categories), read at `observed`
        (bool [N]; None: every node; NaN allowed elsewhere).  The Laplace approximation of the latent posterior under a
        cumulative-logit likelihood with the fixed cutpoints (None: ordinal.ordinal_cutpoints of the observed labels), an
        ordinal.OrdinalLaplaceFit (mode, latent variances and samples, category probabilities); kw as
        ordinal.laplace_fit_ordinal.  The Gaussian likelihood's noise is not used."""
        from ..ordinal import laplace_fit_ordinal
        desc, _, y = self._sampling_args()
        return laplace_fit_ordinal(desc, y, num_categories, cutpoints, observed, **kw)

    def spectral_laplace_posterior(self, observed=None, family="bernoulli", **kw):
        """The Laplace fit of train_targets through the spectral kernel K = s Z Z^T, which predicts at points that were not in
        the graph: a spectral_laplace.SpectralLaplaceFit bound to the kernel, whose latent / predict_* methods take points
        x [T, d] (or their feature rows).  Z = base_kernel.features(train_x), s = covar_module.outputscale; family "bernoulli",
        "poisson", "binomial", "negative_binomial" or "ordinal"; train_targets are read at `observed` (bool [N]; None: every
        node; NaN allowed elsewhere); kw as spectral_laplace.spectral_laplace_fit (exposure, trials, dispersion, num_categories,
        cutpoints, mean, rtol, max_newton, w0).  Needs eval(): the eigenpairs are computed there.  The Gaussian likelihood's
        noise is not used."""
        from ..spectral_laplace import spectral_laplace_fit
        if self.labeled is not None:
            raise NotImplementedError("the spectral Laplace fit of semi-supervised (Schur-complement) models is not supported")
        kernel = self.base_kernel
        if getattr(kernel, "eigvec", None) is None:
            raise RuntimeError("spectral_laplace_posterior needs the kernel's eigenpairs: call model.eval() first")
        for name in ("outputscale", "kernel"):
            if name in kw:
                raise ValueError("%s is the model's own: spectral_laplace_posterior takes none" % name)
        with torch.no_grad():
            Z = kernel.features(self.train_inputs[0])
            s = float(self.covar_module.outputscale) if hasattr(self.covar_module, "outputscale") else 1.0
        fit = spectral_laplace_fit(Z, self.train_targets, observed, family, outputscale=s, **kw)
        fit.kernel = kernel
        return fit

    def _laplace_fit(self, observed, family, **kw):
        """The node fit of train_targets for a family of families.TABLE, by the fitter its record names; kw carries what the record
        says the family needs (num_categories, num_classes) and the fitter's other keywords."""
        from .. import families
        rec = families.fit_family(family)
        families.check_needs(rec, kw)
        desc, _, y = self._sampling_args()
        return families.fitter(rec)(desc, y, observed=observed, **kw)

    def laplace_evidence(self, observed=None, family="bernoulli", **kw):
        """Fit the nodes (_laplace_fit: any family of families.TABLE) and return the Laplace approximation of
        log p(train_targets[observed]), an evidence.LaplaceEvidence.  kw: the arguments of the family's fit (those of the fitter
        its record names: exposure, trials, mean, f0, tolerances, ...) go to it, the others to the evidence function the record
        names (num_probes, steps, seed, method, ...).  max_iter is an argument of both and goes to the FIT; fit_kw= and
        evidence_kw= (dicts, as utils.laplace_train takes them) name the receiver explicitly and win over the split:
        evidence_kw=dict(max_iter=...) caps the evidence's solves.  Where a kernel hyper-parameter requires grad, value carries
        d log Z / d theta.  A family with an extra parameter (the record's `extra`: cutpoints, dispersion) takes it as a number
        or a tensor, or live: as a module (ordinal.CutpointParameter, counts.DispersionParameter) or a float64 tensor that
        requires grad; the fit then runs at the detached values and value carries the derivative in the parameter as well."""
        from .. import families
        rec = families.fit_family(family)
        kw = dict(kw)
        fit_kw, evidence_kw = dict(kw.pop("fit_kw", None) or {}), dict(kw.pop("evidence_kw", None) or {})
        names = families.fit_keywords(rec)
        fit_kw = dict({k: v for k, v in kw.items() if k in names}, **fit_kw)
        evidence_kw = dict({k: v for k, v in kw.items() if k not in names}, **evidence_kw)
        fit_kw, live = families.split_live(rec, fit_kw)
        for name, value in live.items():
            evidence_kw.setdefault(name, value)
        fit = self._laplace_fit(observed, family, **fit_kw)
        return families.evidence_of(rec)(fit, operator=self.precision(noise=False), **evidence_kw)

    # ------------------------------------------------------------------ riemann_gp.py:41-43
    def modulation(self, x):
        edge_value, _ = self.base_kernel.knn.search(x, 1)
        k = self.base_kernel
        return bump_function(edge_value.sqrt().squeeze(-1), k.bump_scale * float(k.graphbandwidth.detach().reshape(-1)[0]), k.bump_decay)

    # ------------------------------------------------------------------ the ExactGP prediction, spelled out
    def _scale_noise(self):
        s = float(self.covar_module.outputscale.detach()) if hasattr(self.covar_module, "outputscale") else 1.0
        nz = self.likelihood.noise.detach().reshape(-1)
        if nz.numel() != 1:
            # per-node noise is the precision-form sampler's (sampling.posterior_mean / posterior_samples with noise [n])
            raise NotImplementedError("per-node likelihood noise is not supported by the spectral posterior or training")
        return s, float(nz[0])

    def _train_cache(self):
        if self._cache is None:
            x, y = self.train_inputs[0], self.train_targets
            s, n = self._scale_noise()
            Z = self.base_kernel.features(x)
            c = float(self.mean_constant.detach())
            from ..solvers import woodbury
            wd = woodbury(Z, y - c, s, n)                              # (K + n I)^-1 (y - c) on the m x m root
            G, Lc, alpha = wd["G"], wd["Lc"], wd["alpha"]
            m = G.shape[0]
            # mean(x*) = c + Z* w,  w = s Z^T alpha = s (Z^T v - G t) / n = t   [(G + (n/s) I) t = Z^T v]
            w = wd["t"].squeeze(-1)
            # cov(x*) = s Z* M Z*^T with M = I - (s/n)(G - G C^-1 G)
            M = torch.eye(m, dtype=torch.float64, device=G.device) - (s / n) * (G - G @ torch.cholesky_solve(G, Lc))
            self._cache = dict(Z=Z, w=w.float(), M=(0.5 * (M + M.t())).float(), s=s, n=n, c=c, alpha=alpha)
        return self._cache

    def __call__(self, x):
        """Posterior of the latent function at x (eval mode), as `self(x)` does for an ExactGP."""
        from ..solvers import kernel_block
        _lib.require_device(x)
        cache = self._train_cache()
        Zs = self.base_kernel.features(x)
        mean = cache["c"] + Zs @ cache["w"]
        covar = kernel_block(Zs @ cache["M"], Zs, cache["s"])         # T x T block on the MFMA
        return _Posterior(mean, 0.5 * (covar + covar.t()))

    def _noisy(self, post, noise):
        eye = torch.eye(post.mean.shape[0], device=post.mean.device)
        return _Posterior(post.mean, post.covariance_matrix + noise * eye)

    # ------------------------------------------------------------------ riemann_gp.py:45-75
    def posterior(self, x, noisy_posterior=False, base_model=None):
        geom = self(x)
        self.posterior_geom = self._noisy(geom, self._scale_noise()[1]) if noisy_posterior else geom
        for name in ("posterior_base", "base_scale"):
            if hasattr(self, name):
                delattr(self, name)
        if base_model is not None:
            base = base_model(x)
            if noisy_posterior and hasattr(base_model, "likelihood"):
                base = self._noisy(base, float(base_model.likelihood.noise.detach().reshape(-1)[0]))
            self.posterior_base = base
            self.base_scale = 1 - self.modulation(x)
        return self

    @property
    def posterior_mean(self):
        mean = self.posterior_geom.mean.clone()
        if hasattr(self, "posterior_base"):
            mean += self.base_scale * self.posterior_base.mean
        return mean

    @property
    def posterior_covar(self):
        covar = self.posterior_geom.covariance_matrix.clone()
        if hasattr(self, "posterior_base"):
            covar += torch.outer(self.base_scale, self.base_scale) * self.posterior_base.covariance_matrix
        return covar

    @property
    def posterior_stddev(self):
        stddev = self.posterior_geom.stddev.clone()
        if hasattr(self, "posterior_base"):
            stddev += self.base_scale * self.posterior_base.stddev
        return stddev


class EuclideanGP(torch.nn.Module):
    """Exact GP with a constant mean and an RBF kernel on the ambient coordinates: the `base_model` of
    the hybrid posterior (benchmark/*.py of the reference build a gpytorch ExactGP for it).  Dense
    Cholesky through torch: sized for the labelled subset, not the hot path."""

    def __init__(self, train_x, train_y, likelihood, lengthscale=1.0, outputscale=1.0, mean=0.0):
        super().__init__()
        self.train_x, self.train_y, self.likelihood = train_x, train_y, likelihood
        self.lengthscale, self.outputscale, self.mean = float(lengthscale), float(outputscale), float(mean)
        self._chol = None

    def _k(self, a, b):
        d2 = torch.cdist(a.double(), b.double()).square()
        return self.outputscale * torch.exp(-0.5 * d2 / self.lengthscale ** 2)

    def __call__(self, x):
        n = float(self.likelihood.noise.detach().reshape(-1)[0])
        if self._chol is None:
            K = self._k(self.train_x, self.train_x)
            self._chol = torch.linalg.cholesky(K + n * torch.eye(K.shape[0], dtype=K.dtype, device=K.device))
            self._alpha = torch.cholesky_solve((self.train_y.double() - self.mean).unsqueeze(-1), self._chol).squeeze(-1)
        Ks = self._k(x, self.train_x)
        mean = self.mean + Ks @ self._alpha
        cov = self._k(x, x) - Ks @ torch.cholesky_solve(Ks.t(), self._chol)
        return _Posterior(mean.float(), cov.float())
