"""Time the marginal posterior variance in precision form (manifold_gp_amd/sampling.py::posterior_variance) on the 60k
manifold_784 graph (k = 50, random walk; nu = 2 and 3; noise 1e-2; every node or 10 % of the nodes observed) at S = 64 and
256: the wall time of the call, the event time of each of its two kernels alone (mgp_operator_diag_exact, mgp_row_moments),
the share of the CG solves, and, per method, the median and the 95th percentile of se / var over the nodes -- there is no
float64 truth at this size, so se / var says which regime the workload is in.  Prints one JSON line.

    python tools/time_variance.py [--reps 5]
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


def _case(desc, noise, observed, S_list, reps):
    from manifold_gp_amd import sampling
    from manifold_gp_amd.solvers import cg_solve
    ob = sampling._observation(desc, noise, observed)
    P = sampling._check_desc(desc)
    s = float(noise) if ob is None else ob.s_ref
    dsys = desc.with_(form=2, noise=s) if ob is None else ob.descriptor(desc)
    kw = sampling._solve_kw(1e-6, 1, 5000)
    if ob is not None:
        kw["jacobi"] = sampling.OBSERVED_JACOBI[0]
    out = dict(diag_exact_us=round(_events_ms(lambda: sampling.operator_diag_exact(dsys), reps) * 1e3, 2), S={})
    rdiag = sampling.operator_diag_exact(dsys).reciprocal()
    for S in S_list:
        r = dict(wall_ms=round(_wall_ms(lambda: sampling.posterior_variance(desc, noise, S, 5, observed=observed), reps), 3))
        solve_ms = moments_ms = 0.0
        for c0 in range(0, S, sampling.CHUNK):
            C = min(sampling.CHUNK, S - c0)
            p = sampling._perturbation(desc, P, ob, s, C, 5, c0)
            X, its, _ = cg_solve(dsys, p, **kw)
            acc = torch.zeros(desc.n, 2, dtype=torch.float64, device=p.device)
            solve_ms += _wall_ms(lambda: cg_solve(dsys, p, **kw), reps)
            moments_ms += _events_ms(lambda: sampling.row_moments(acc, X, None, rdiag, p), reps)
            r["cg_iters"] = int(its)
        r["row_moments_us"] = round(moments_ms * 1e3, 2)
        r["solve_share"] = round(solve_ms / r["wall_ms"], 4)
        for method in ("rao-blackwell", "samples"):
            var, se = sampling.posterior_variance(desc, noise, S, 5, observed=observed, method=method)
            q = (se / var).cpu().numpy()
            r[method] = dict(se_over_var_median=float("%.4g" % np.median(q)), se_over_var_p95=float("%.4g" % np.percentile(q, 95)))
        out["S"][str(S)] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    res = dict(tool="time_variance")
    n = 60000
    x_np, y_np, _ = synth.manifold_784(n)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    obs10 = torch.from_numpy(np.random.default_rng(10).random(n) < 0.1).to(dev)
    for nu in (2, 3):
        kern = mgp.kernels.RiemannMaternKernel(nu=nu, x=x, nearest_neighbors=50, laplacian_normalization="randomwalk",
                                               num_modes=20).to(dev)
        kern.initialize(graphbandwidth=0.3, lengthscale=3.0)
        model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
        desc, noise, _ = model._sampling_args()
        for name, observed in (("observed_100", None), ("observed_10", obs10)):
            res["manifold784_60k_nu%d_%s" % (nu, name)] = _case(desc, noise, observed, (64, 256), args.reps)
        del model, kern
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
