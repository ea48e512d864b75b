"""Time the posterior on a subset of nodes (operator form 3, A = diag(w) + s Q2; manifold_gp_amd/sampling.py) on the 60k
manifold_784 graph (k = 50, random walk, nu = 2, noise 1e-2): CG iterations and ms of posterior_mean at 100 % (form 3 with
w = 1 against form 2), 50 % and 10 % observed, Jacobi off and on; posterior_samples ms at S = 1, 16, 64, 256; one operator
apply of form 3 against form 2 at C = 1, 16, 256.  Prints one JSON line.

    python tools/time_observed.py [--reps 5] [--fracs 1.0,0.5,0.1]
"""
import argparse
import json
import os
import sys
import time

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
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fracs", default="1.0,0.5,0.1")
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd import sampling, solvers
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    dev = torch.device("cuda:0")
    n, k, nu, eps, kappa, s, noise = 60000, 50, 2, 0.3, 3.0, 1.0, 1e-2
    x_np, y_np, _ = synth.manifold_784(n)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=k, laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=eps, lengthscale=kappa)
    model = RiemannGP(x, y, GaussianLikelihood(noise).to(dev), ScaleKernel(kern, s).to(dev)).to(dev)
    desc = model.precision(noise=False)._descriptor()
    out = dict(n=n, k=k, nu=nu, noise=noise, mean={}, samples={}, apply_us={})
    rng = np.random.default_rng(0)
    kw = dict(tol=1e-5, stop_mode=1, max_iter=5000)
    for frac in [float(f) for f in args.fracs.split(",")]:
        obs = torch.from_numpy(rng.random(n) < frac).to(dev) if frac < 1.0 else torch.ones(n, dtype=torch.bool, device=dev)
        ob = sampling._observation(desc, torch.full((n,), noise, device=dev), obs)
        d3 = ob.descriptor(desc)
        rhs = ob.weighted_targets(y.view(-1, 1))
        for jac in (False, True):
            key = "%g%%/jacobi=%d" % (100 * frac, jac)
            its = solvers.cg_solve(d3, rhs, jacobi=jac, **kw)[1]
            ms = _wall_ms(lambda: solvers.cg_solve(d3, rhs, jacobi=jac, **kw), args.reps)
            out["mean"][key] = dict(iters=int(its), ms=round(ms, 3))
        if frac == 1.0:
            d2 = desc.with_(form=2, noise=noise)
            for jac in (False, True):
                its = solvers.cg_solve(d2, y.view(-1, 1), jacobi=jac, **kw)[1]
                ms = _wall_ms(lambda: solvers.cg_solve(d2, y.view(-1, 1), jacobi=jac, **kw), args.reps)
                out["mean"]["form2/jacobi=%d" % jac] = dict(iters=int(its), ms=round(ms, 3))
            for C in (1, 16, 256):
                X = torch.randn(n, C, device=dev)
                out["apply_us"]["C=%d" % C] = dict(
                    form2=round(1e3 * _events_ms(lambda: d2.apply(X), args.reps), 1),
                    form3=round(1e3 * _events_ms(lambda: d3.apply(X), args.reps), 1))
        obs_arg = None if frac == 1.0 else obs
        for S in (1, 16, 64, 256):      # (form 3 throughout: a noise vector; Jacobi as sampling.OBSERVED_JACOBI says)
            ms = _wall_ms(lambda: sampling.posterior_samples(desc, y, torch.full((n,), noise, device=dev), S, 7,
                                                             observed=obs_arg), max(1, args.reps // 2))
            out["samples"]["%g%%/S=%d" % (100 * frac, S)] = round(ms, 2)
        solvers.clear_plan_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
