"""Time exact GMRF sampling (manifold_gp_amd/sampling.py): the noise kernel (mgp_gmrf_noise, with and without the edge
term) and the end-to-end RiemannGP.sample_prior / sample_posterior, on the 60k manifold_784 graph (k = 50, random walk,
nu = 2; S = 1, 16, 64, 256; the posterior at S = 64 also with nu = 3, whose noise carries the edge term) and on the 1M swiss
roll (k = 64, symmetric, nu = 2; S = 1, 16).  Prints one JSON line.

    python tools/time_sampling.py [--skip-1m] [--reps 5]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _events_ms(fn, reps):
    """Median device time of fn() over reps (one warm-up call first)."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def _case(model, S_list, reps):
    from manifold_gp_amd import sampling
    desc = model.precision(noise=False)._descriptor()
    data = desc.data
    nnz, n = data.graph.nnz, data.graph.n
    noise = float(model.likelihood.noise.detach().reshape(-1)[0])
    out = dict(n=n, nnz=nnz, nu=int(desc.nu), S={})
    for S in S_list:
        r = {}
        quads = (S + 3) // 4
        for edges in (False, True):
            ms = _events_ms(lambda: sampling.gmrf_noise(data, S, 1234, node_coef=1.0, edges=edges), reps)
            key = "noise_edges_us" if edges else "noise_nodes_us"
            r[key] = round(ms * 1e3, 2)
            if edges:
                r["entry_quads_per_s"] = float("%.4g" % (nnz * quads / (ms * 1e-3)))
        r["sample_prior_ms"] = round(_wall_ms(lambda: model.sample_prior(S, seed=5), reps), 3)
        r["sample_posterior_ms"] = round(_wall_ms(lambda: model.sample_posterior(S, seed=5), reps), 3)
        # noise share of a posterior call: the noise launches it makes (w or g, then w2), each timed on its own
        edges = desc.nu % 2 == 1
        share_ms = 0.0
        for c0 in range(0, S, sampling.CHUNK):
            C = min(sampling.CHUNK, S - c0)
            share_ms += _events_ms(lambda: sampling.gmrf_noise(data, C, 5, c0, node_coef=1.0, edges=edges), reps)
            share_ms += _events_ms(lambda: sampling.gmrf_noise(data, C, 5, c0, node_coef=noise ** 0.5, tag=2), reps)
        r["posterior_noise_share"] = round(share_ms / r["sample_posterior_ms"], 4)
        out["S"][str(S)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-1m", action="store_true")
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    res = dict(tool="time_sampling")
    # ---- 60k manifold_784 (the workload of tests/test_gpu_configs.py's C3-size manifold test)
    x_np, y_np, _ = synth.manifold_784(60000)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    for nu, S_list in ((2, (1, 16, 64, 256)), (3, (64,))):
        kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=50, laplacian_normalization="randomwalk",
                                               num_modes=20).to(dev)
        kern.initialize(graphbandwidth=0.3, lengthscale=3.0)
        model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
        res["manifold784_60k_nu%d" % nu] = _case(model, S_list, args.reps)
        del model, kern
        torch.cuda.empty_cache()
    # ---- 1M swiss roll (bench.py's s5 workload: k = 64, symmetric, nu = 2, eps = 3 eps_min)
    if not args.skip_1m:
        x_np, y_np = synth.swiss_roll(1000000)
        x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
        kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=64, laplacian_normalization="symmetric",
                                               num_modes=20).to(dev)
        D1, _ = kern.knn.search(x, 2)
        eps = 3.0 * synth.bandwidth_rule(D1[:, 1].cpu().numpy(), 0.0)[1]
        kern.initialize(graphbandwidth=eps, lengthscale=1.0)
        model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
        res["swissroll_1m_nu2"] = _case(model, (1, 16), max(2, args.reps // 2))
        res["swissroll_1m_nu2"]["eps"] = eps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
