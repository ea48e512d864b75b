"""Time the C-class Laplace classification (classification.laplace_fit_multiclass) on the 60k manifold_784 graph (k = 50, random
walk, nu = 2; C = 10 classes: the quantile bins of the roll coordinate, 10 % of the nodes observed, 5 % of the labels moved to
another class) at two output scales: the wall time of the fit with its Newton and CG iteration counts, the time per CG step of
mgp_softmax_cg, the event times of mgp_softmax_site, of mgp_softmax_hessian_add and of the operator chain on C columns (what
is left of a step is the update launch and the host's share), and -- in the same process, alternating with the HIP solver --
the same recurrence restated in torch ops (desc.apply plus row ops, scalars kept on the device, one host read per check_every
steps).  The block path (mgp_softmax_cg_block, block=): predict_proba(16, seed=3) with block=None and with block=16 in the same
process, warmed, taking turns; one block solve of 16 posterior right-hand sides at the mode's weights (iterations per sample,
wall time, time per step issued); and the largest difference between the two estimates of the class probabilities.
Prints one JSON line.  Nothing here is an acceptance bar.

    python tools/time_softmax.py [--reps 5]
    python tools/time_softmax.py --trace-block        # only warmed block solves at outputscale 1: the program of a kernel trace
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

from tools.time_sampling import _events_ms, _wall_ms  # noqa: E402

C = 10


def torch_cg(desc, pi, B, tol, max_iter=5000, check_every=8):
    """The recurrence of mgp_softmax_cg in torch ops: (X, steps run).  The scalars stay on the device; a converged solve keeps
    stepping with alpha = 0 until the next host read."""
    X, R = torch.zeros_like(B), B.clone()
    P, S = torch.zeros_like(B), torch.zeros_like(B)
    bb = gamma_old = alpha_old = None
    tol2 = tol * tol
    for step in range(1, max_iter + 2):
        W = desc.apply(R)
        W += pi * R - pi * (pi * R).sum(1, keepdim=True)
        Rd = R.double()
        gamma, delta = (Rd * Rd).sum(), (Rd * W.double()).sum()
        if step == 1:
            bb = gamma
            beta = torch.zeros_like(gamma)
            alpha = gamma / delta
        else:
            beta = gamma / gamma_old
            alpha = gamma / (delta - beta * gamma / alpha_old)
        live = gamma > tol2 * bb
        alpha = torch.where(live, alpha, torch.zeros_like(alpha))
        P = R + beta.float() * P
        S = W + beta.float() * S
        X = X + alpha.float() * P
        R = R - alpha.float() * S
        gamma_old, alpha_old = gamma, torch.where(live, alpha, alpha_old if alpha_old is not None else alpha)
        if step % check_every == 0 and not bool(live):
            return X, step
    return X, max_iter + 1


def _alternate(fns, reps):
    """Median wall ms of each function, the functions taking turns (one warm-up round first)."""
    ts = [[] for _ in fns]
    for rep in range(reps + 1):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


BLOCK = 16


def _block_rhs(fit, b, seed):
    """The right-hand sides of the first block of b posterior samples, [n, b, C], as MulticlassLaplaceFit._samples builds them."""
    from manifold_gp_amd import classification as cl, sampling
    desc, n = fit.desc, fit.desc.n
    P = sampling._check_desc(desc)
    z = sampling._precision_chunk(desc, P, b * C, seed, 0).view(n, b, C)
    eps = sampling.gmrf_noise(desc.data, b * C, seed, 0, tag=2).view(n, b, C)
    return z + cl.softmax_noise_factor(fit.pi[:, None, :], eps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-block", action="store_true",
                    help="run two block solves of 16 samples at outputscale 1 and nothing else (for a kernel trace of a block step)")
    args = ap.parse_args()
    import manifold_gp_amd as mgp
    from manifold_gp_amd import classification as cl
    from manifold_gp_amd.models import GaussianLikelihood, RiemannGP, ScaleKernel
    from tools import synth
    dev = torch.device("cuda:0")
    warnings.simplefilter("ignore")
    n = 60000
    x_np, y_np, (roll, _) = synth.manifold_784(n)
    rng = np.random.default_rng(7)
    t = np.searchsorted(np.quantile(roll, np.arange(1, C) / C), roll, side="right")
    t = np.where(rng.random(n) < 0.05, (t + rng.integers(1, C, n)) % C, t)
    obs = torch.from_numpy(rng.random(n) < 0.1).to(dev)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(t.astype(np.float32)).to(dev)
    kern = mgp.kernels.RiemannMaternKernel(nu=2, x=x, nearest_neighbors=50, laplacian_normalization="randomwalk",
                                           num_modes=20).to(dev)
    kern.initialize(graphbandwidth=0.3, lengthscale=3.0)
    model = RiemannGP(x, y, GaussianLikelihood(1e-2).to(dev), ScaleKernel(kern, 1.0).to(dev)).to(dev)
    desc0, _, _ = model._sampling_args()
    res = dict(tool="time_softmax", n=n, classes=C)
    for outputscale in (1.0,) if args.trace_block else (1.0, 100.0):
        desc = desc0.with_(scale=float(desc0.scale) / outputscale)      # the precision of outputscale x the kernel
        fit = cl.laplace_fit_multiclass(desc, y, C, obs)
        if args.trace_block:
            rhs = _block_rhs(fit, BLOCK, 3)
            for _ in range(2):
                _, its, _ = cl.softmax_cg_solve_block(desc, fit.pi, rhs, tol=1e-5)
            torch.cuda.synchronize()
            print(json.dumps(dict(tool="time_softmax", trace_block=True, iterations=its)))
            return
        r = dict(converged=bool(fit.converged), newton_steps=fit.iterations, cg_iterations=[h[3] for h in fit.history],
                 steps=[h[2] for h in fit.history], max_abs_mode=round(float(fit.mean.abs().max()), 3),
                 fit_wall_ms=round(_wall_ms(lambda: cl.laplace_fit_multiclass(desc, y, C, obs), args.reps), 3))
        f, pi = fit.mean, fit.pi
        qf = cl._q2(desc, f)
        lab = fit.labels
        r["site_us"] = round(_events_ms(lambda: cl.softmax_site(f, qf, lab, obs), args.reps) * 1e3, 2)
        r["apply_f64_us"] = round(_events_ms(lambda: cl._q2(desc, f), args.reps) * 1e3, 2)
        Y = torch.zeros_like(f)
        r["hessian_add_us"] = round(_events_ms(lambda: cl.softmax_hessian_add(pi, f, Y), args.reps) * 1e3, 2)
        r["apply_f32_us"] = round(_events_ms(lambda: desc.apply(f), args.reps) * 1e3, 2)
        # one Newton system at the mode's weights: the first step's right-hand side, HIP and torch taking turns
        B = cl.softmax_site(torch.zeros_like(f), None, lab, obs)[1]
        X, its, resid = cl.softmax_cg_solve(desc, pi, B, tol=1e-3)
        Xt, steps_t = torch_cg(desc, pi, B, 1e-3)
        hip_ms, torch_ms = _alternate([lambda: cl.softmax_cg_solve(desc, pi, B, tol=1e-3), lambda: torch_cg(desc, pi, B, 1e-3)],
                                      args.reps)
        steps_h = its + 1                                                # the deciding step runs its apply too
        steps_h = -(-steps_h // 8) * 8                                   # launches are issued up to the next host read
        r.update(solve_iterations=its, solve_resid=round(resid, 6), solve_hip_ms=round(hip_ms, 3), solve_torch_ms=round(torch_ms, 3),
                 step_hip_us=round(hip_ms * 1e3 / steps_h, 2), step_torch_us=round(torch_ms * 1e3 / steps_t, 2),
                 steps_issued_hip=steps_h, steps_run_torch=steps_t,
                 torch_vs_hip_solution=float((Xt - X).abs().max() / X.abs().max()))
        prob = fit.predict_proba(16, seed=3)
        r["predict_proba_16_wall_ms"] = round(_wall_ms(lambda: fit.predict_proba(16, seed=3), 1), 3)
        r["accuracy_unobserved"] = round(float((prob.argmax(1) == y.long())[~obs].float().mean()), 4)
        # the block path against the per-sample path of the same tree, warmed, taking turns
        prob_b = fit.predict_proba(BLOCK, seed=3, block=BLOCK)
        single_ms, block_ms = _alternate([lambda: fit.predict_proba(BLOCK, seed=3), lambda: fit.predict_proba(BLOCK, seed=3, block=BLOCK)],
                                         args.reps)
        rhs = _block_rhs(fit, BLOCK, 3)
        Xb, its_b, resid_b = cl.softmax_cg_solve_block(desc, pi, rhs, tol=1e-5)
        solve_b_ms = _wall_ms(lambda: cl.softmax_cg_solve_block(desc, pi, rhs, tol=1e-5), args.reps)
        steps_b = -(-(max(its_b) + 1) // 8) * 8                          # launches are issued up to the next host read
        r["block"] = dict(samples=BLOCK, predict_proba_single_ms=round(single_ms, 3), predict_proba_block_ms=round(block_ms, 3),
                          single_over_block=round(single_ms / block_ms, 3), max_abs_prob_diff=float((prob_b - prob).abs().max()),
                          accuracy_unobserved=round(float((prob_b.argmax(1) == y.long())[~obs].float().mean()), 4),
                          solve_iterations=its_b, solve_max_resid=round(max(resid_b), 8), solve_ms=round(solve_b_ms, 3),
                          steps_issued=steps_b, step_us=round(solve_b_ms * 1e3 / steps_b, 2))
        res["outputscale_%g" % outputscale] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
