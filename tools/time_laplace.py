"""Time the Laplace classification (manifold_gp_amd/classification.py) on the 60k manifold_784 graph (k = 50, random walk,
nu = 2; labels: the targets above their median, 10 % of the nodes observed, 5 % of the labels flipped) at two output
scales: the wall time of laplace_fit with its Newton and CG iteration counts, the event time of mgp_bernoulli_site against
its 18 B per node at the HBM rate, of the float64 apply behind it, of mgp_bernoulli_predict at K = 129, and the wall time of
predict_proba at S = 64.  Prints one JSON line.  Nothing here is an acceptance bar.

    python tools/time_laplace.py [--reps 5]
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

HBM_BYTES_PER_S = 8.0e12     # MI355X datasheet rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd import classification as cl
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    n = 60000
    x_np, y_np, _ = synth.manifold_784(n)
    rng = np.random.default_rng(7)
    t = y_np > np.median(y_np)
    t = np.where(rng.random(n) < 0.05, ~t, t).astype(np.float32)
    obs = torch.from_numpy(rng.random(n) < 0.1).to(dev)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(t).to(dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=50, laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=0.3, lengthscale=3.0)
    model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
    desc0, _, _ = model._sampling_args()
    res = dict(tool="time_laplace", n=n)
    for outputscale in (1.0, 100.0):
        desc = desc0.with_(scale=float(desc0.scale) / outputscale)      # the precision of outputscale x the kernel
        fit = cl.laplace_fit(desc, y, obs)
        r = dict(converged=bool(fit.converged), newton_steps=fit.iterations, cg_iterations=[h[3] for h in fit.history],
                 steps=[h[2] for h in fit.history], max_abs_mode=round(float(fit.mean.abs().max()), 3),
                 fit_wall_ms=round(_wall_ms(lambda: cl.laplace_fit(desc, y, obs), args.reps), 3))
        f = fit.mean
        qf = cl._q2(desc, f)
        site_ms = _events_ms(lambda: cl.bernoulli_site(f, qf, y, obs), args.reps)
        r["site_us"] = round(site_ms * 1e3, 2)
        r["site_share_of_hbm_rate"] = round(18.0 * n / (site_ms * 1e-3) / HBM_BYTES_PER_S, 4)
        r["apply_f64_us"] = round(_events_ms(lambda: cl._q2(desc, f), args.reps) * 1e3, 2)
        r["apply_f32_us"] = round(_events_ms(lambda: desc.apply(f), args.reps) * 1e3, 2)
        prob, var = fit.predict_proba(64, seed=3)
        r["predict_us"] = round(_events_ms(lambda: cl.bernoulli_predict(f, var), args.reps) * 1e3, 2)
        r["predict_proba_wall_ms"] = round(_wall_ms(lambda: fit.predict_proba(64, seed=3), args.reps), 3)
        r["accuracy_unobserved"] = round(float(((prob > 0.5).float() == y)[~obs].float().mean()), 4)
        res["outputscale_%g" % outputscale] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
