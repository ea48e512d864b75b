"""Time the count fits (manifold_gp_amd/counts.py) on the 60k manifold_784 graph (k = 50, random walk, nu = 2; 10 % of the
nodes observed; Poisson counts with exposures in [0.5, 20] and binomial counts out of 1 .. 39 trials, both from 1.2 x the
standardised targets) at two output scales: the wall time of laplace_fit_counts with its Newton and CG iteration counts, the
event time of the count_site call next to bernoulli_site in the same process, the wall time of predict_mean at S = 64, and the
event times of the predictive pmf of the counts 0 .. 512 at every node (60k x 513 quadratures, P = 65 and 129) and of the log
density of the node's own count, both with predict_mean's latent variance.
Prints one JSON line.  Nothing here is an acceptance bar.

    python tools/time_counts.py [--reps 5]
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.time_sampling import _events_ms, _wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd import classification as cl, counts as ct
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    n = 60000
    x_np, y_np, _ = synth.manifold_784(n)
    rng = np.random.default_rng(11)
    ftrue = 1.2 * (y_np - y_np.mean()) / y_np.std()
    E = rng.uniform(0.5, 20.0, n)
    obs_np = rng.random(n) < 0.1
    y_pois = rng.poisson(E * np.exp(1.0 + ftrue)).astype(np.float32)
    N = rng.integers(1, 40, n)
    y_bin = rng.binomial(N, 1.0 / (1.0 + np.exp(-ftrue))).astype(np.float32)
    x, obs = torch.from_numpy(x_np).to(dev), torch.from_numpy(obs_np).to(dev)
    data = {"poisson": (torch.from_numpy(y_pois).to(dev), dict(exposure=torch.from_numpy(E).to(dev))),
            "binomial": (torch.from_numpy(y_bin).to(dev), dict(trials=torch.from_numpy(N.astype(np.float32)).to(dev)))}
    labels = (data["binomial"][0] * 2 > data["binomial"][1]["trials"]).float()       # 0/1 labels for the bernoulli_site call
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=50, laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=0.3, lengthscale=3.0)
    model = RiemannGP(x, data["poisson"][0], GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
    desc0, _, _ = model._sampling_args()
    res = dict(tool="time_counts", n=n)
    for outputscale in (1.0, 100.0):
        desc = desc0.with_(scale=float(desc0.scale) / outputscale)      # the precision of outputscale x the kernel
        for family, (y, kw) in data.items():
            fit = ct.laplace_fit_counts(desc, y, obs, family=family, **kw)
            r = dict(converged=bool(fit.converged), newton_steps=fit.iterations, cg_iterations=[h[3] for h in fit.history],
                     steps=[h[2] for h in fit.history], max_abs_mode=round(float(fit.mean.abs().max()), 3),
                     prior_mean=round(fit.prior_mean, 4), s_ref=fit.s_ref,
                     fit_wall_ms=round(_wall_ms(lambda: ct.laplace_fit_counts(desc, y, obs, family=family, **kw), args.reps), 3))
            f = fit.mean
            qf = cl._q2(desc, f)
            r["count_site_us"] = round(_events_ms(lambda: ct.count_site(f, qf, fit.y, fit._aux, obs, fit.s_ref, fit.prior_mean,
                                                                        family), args.reps) * 1e3, 2)
            r["bernoulli_site_us"] = round(_events_ms(lambda: cl.bernoulli_site(f, qf, labels, obs), args.reps) * 1e3, 2)
            mean, var, lv = fit.predict_mean(64, seed=3)
            r["predict_mean_wall_ms"] = round(_wall_ms(lambda: fit.predict_mean(64, seed=3), args.reps), 3)
            for points in (65, 129):
                r["predict_pmf_513_counts_p%d_ms" % points] = round(_events_ms(
                    lambda: fit.predict_pmf(512, points=points, variance=lv), args.reps), 3)
            r["predict_log_density_us"] = round(_events_ms(lambda: fit.predict_log_density(y, variance=lv), args.reps) * 1e3, 2)
            truth = E * np.exp(1.0 + ftrue) if family == "poisson" else N / (1.0 + np.exp(-ftrue))
            # (exposure and trials are given at every node.)  The Poisson predictive mean carries exp(v / 2): at a prior variance
            # of 100 it is far above the median of the predictive rate, which is what map_mean follows
            for name, m in (("predict_mean", mean), ("map_mean", fit.map_mean())):
                rel = (m.cpu().numpy() - truth)[~obs_np] / truth[~obs_np]
                r["median_rel_error_unobserved_" + name] = round(float(np.median(np.abs(rel))), 4)
            r["median_latent_variance_unobserved"] = round(float(lv[~obs].median()), 4)
            res["%s_outputscale_%g" % (family, outputscale)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
