"""Time the Laplace evidence (manifold_gp_amd/evidence.py) on the 60k manifold_784 workload of tools/time_counts.py (k = 50,
random walk, nu = 2; 10 % of the nodes observed; 0/1 labels, Poisson and binomial counts, and three classes for the softmax fit,
whose evidence is evidence.softmax_evidence): the wall time of the evidence value
with 16 probes (method "slq": m = 6000 is above the dense threshold), of the value with its hyper-parameter gradient (backward
included), and of one laplace_train epoch, each the median of --reps in one warmed process, and the share of each spent inside
cg_solve (a second, instrumented pass that synchronises around every solve).  Prints one JSON line.  Nothing here is an
acceptance bar.

    python tools/time_evidence.py [--reps 5] [--families bernoulli,poisson,binomial,multiclass]
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

from tools.time_sampling import _wall_ms  # noqa: E402


class _SolveClock:
    """Replaces solvers.cg_solve, evidence._solve64 (the float64 solves of the gradient, which go to their plan directly) and
    classification.softmax_cg_solve_block (the coupled solves of the softmax family) by wrappers that add up the synchronised
    wall time of the solves."""

    def __init__(self):
        from manifold_gp_amd import classification, evidence, solvers
        self.targets = [(solvers, "cg_solve", solvers.cg_solve), (evidence, "_solve64", evidence._solve64),
                        (classification, "softmax_cg_solve_block", classification.softmax_cg_solve_block)]
        self.ms, self.calls = 0.0, 0

    def _timed(self, inner):
        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*a, **kw)
            torch.cuda.synchronize()
            self.ms += (time.perf_counter() - t0) * 1e3
            self.calls += 1
            return out
        return timed

    def __enter__(self):
        for mod, name, inner in self.targets:
            setattr(mod, name, self._timed(inner))
        return self

    def __exit__(self, *exc):
        for mod, name, inner in self.targets:
            setattr(mod, name, inner)


def _timed(fn, reps):
    """(median wall ms, share of the instrumented run spent in cg_solve, solves per call)"""
    wall = _wall_ms(fn, reps)
    shares, calls = [], 0
    for _ in range(reps):
        with _SolveClock() as clock:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
        shares.append(clock.ms / total)
        calls = clock.calls
    return round(wall, 3), round(float(np.median(shares)), 3), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--families", default="bernoulli,poisson,binomial,multiclass")
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from manifold_gp_amd.utils import laplace_train
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
    trials = torch.from_numpy(N.astype(np.float32)).to(dev)
    data = {"bernoulli": ((torch.from_numpy(y_bin).to(dev) * 2 > trials).float(), {}),
            "poisson": (torch.from_numpy(y_pois).to(dev), dict(exposure=torch.from_numpy(E).to(dev))),
            "binomial": (torch.from_numpy(y_bin).to(dev), dict(trials=trials)),
            "multiclass": (torch.from_numpy(np.searchsorted(np.quantile(ftrue, [1 / 3, 2 / 3]), ftrue).astype(np.float32)).to(dev),
                           dict(num_classes=3))}
    data = {k: v for k, v in data.items() if k in args.families.split(",")}
    res = dict(tool="time_evidence", n=n, observed=int(obs_np.sum()), probes=16, steps=12)
    for family, (y, kw) in data.items():
        kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=50, laplacian_normalization="randomwalk",
                                               num_modes=20).to(dev)
        kern.initialize(graphbandwidth=0.3, lengthscale=3.0)
        model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
        fit = model._laplace_fit(obs, family, **kw)
        evidence = fit.laplace_evidence if family == "multiclass" else fit.evidence
        ev = evidence()
        r = dict(m=ev.m, method=ev.method, log_z=round(float(ev.value), 3), se=round(ev.se, 3), logdet_b=round(ev.logdet, 3),
                 fit_newton_steps=fit.iterations)

        def with_gradient():
            model.zero_grad()
            evidence(operator=model.precision(noise=False)).value.backward()

        def epoch():
            opt = torch.optim.Adam(model.parameters(), lr=0.0)          # the hyper-parameters stay where they are
            laplace_train(model, opt, observed=obs, family=family, max_iter=0, fit_kw=dict(kw, f0=fit.mean))
        for name, fn in (("value", lambda: evidence()), ("value_and_gradient", with_gradient), ("train_epoch", epoch)):
            r[name + "_wall_ms"], r[name + "_solve_share"], r[name + "_solves"] = _timed(fn, args.reps)
        res[family] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
