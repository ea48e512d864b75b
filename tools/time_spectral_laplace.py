"""Time one Newton evaluation of the spectral Laplace fit (mgp_spectral_site, manifold_gp_amd/spectral_laplace.py) at n = 60 000
rows of m = 100 features, 10 % and 100 % of the rows observed, Bernoulli and Poisson, with and without the Hessian, against the
same quantities written with what the library had before it: torch float64 on the device (Z.double() @ w, the family's
formulas, Z.double().T @ (h[:, None] * Z.double())).  Device events around windows of --calls calls after a warm-up, the entry
point and the baseline alternated window by window in one process, --windows windows each; the median and the spread
(max - min) over the windows per call, and the achieved bytes / s of one pass over Z (4 n m bytes over the time of the call
without a Hessian, which is one pass).  Z is seeded noise of the features' size: the time does not depend on its values.
Prints one JSON line.  Nothing here is an acceptance bar.

    python tools/time_spectral_laplace.py [--n 60000] [--m 100] [--calls 200] [--windows 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _window_us(fn, calls):
    """microseconds per call of `calls` back-to-back calls, by device events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls


def _torch_baseline(Zd, w, family, a, b, obs, mean, hessian):
    """the evaluation with torch float64 on the device; Zd = Z.double() is formed once outside (in the baseline's favour)"""
    f = Zd @ w
    eta = f + mean
    if family == "bernoulli":
        e = torch.exp(-eta.abs())
        d = 1.0 + e
        pi = torch.where(eta >= 0, 1.0 / d, e / d)
        lp = torch.minimum(torch.where(a > 0.5, eta, -eta), torch.zeros_like(eta)) - torch.log1p(e)
        g, h = (a > 0.5).double() - pi, e / (d * d)
    else:
        eta = eta + b
        mu = torch.exp(eta.clamp_max(700.0))
        lp, g, h = a * eta - mu, a - mu, mu
    if obs is not None:
        zero = torch.zeros_like(f)
        lp, g, h = torch.where(obs, lp, zero), torch.where(obs, g, zero), torch.where(obs, h, zero)
    grad = Zd.T @ g
    hess = Zd.T @ (h[:, None] * Zd) if hessian else None
    return f, grad, hess, torch.stack([lp.sum(), f.abs().max()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_spectral_laplace needs the GPU: there is nothing to time without it")
    from manifold_gp_amd.spectral_laplace import spectral_site
    dev = torch.device("cuda:0")
    n, m = args.n, args.m
    rng = np.random.default_rng(5)
    Z = torch.from_numpy((rng.standard_normal((n, m)) / np.sqrt(m)).astype(np.float32)).to(dev)
    w = torch.from_numpy(1.5 * rng.standard_normal(m)).to(dev)
    ftrue = (Z.double() @ w).cpu().numpy()
    E = rng.uniform(0.5, 20.0, n)
    data = {"bernoulli": (torch.from_numpy((rng.random(n) < 1.0 / (1.0 + np.exp(-ftrue))).astype(np.float32)).to(dev), None),
            "poisson": (torch.from_numpy(rng.poisson(E * np.exp(np.minimum(ftrue, 4.0))).astype(np.float32)).to(dev),
                        torch.from_numpy(np.log(E).astype(np.float32)).to(dev))}
    masks = {"10": torch.from_numpy(rng.random(n) < 0.1).to(dev), "100": None}
    Zd = Z.double()
    res = dict(tool="time_spectral_laplace", n=n, m=m, calls_per_window=args.calls, windows=args.windows, pass_bytes=4 * n * m)
    for family, (a, b) in data.items():
        a64, b64 = a.double(), None if b is None else b.double()
        for frac, obs in masks.items():
            r = {}
            for hessian in (True, False):
                kernel = lambda: spectral_site(Z, w, family, a, b, obs, 0.25, None, hessian)          # noqa: E731
                base = lambda: _torch_baseline(Zd, w, family, a64, b64, obs, 0.25, hessian)           # noqa: E731
                got, want = kernel(), base()
                for x, y in zip(got, want):                                                          # the same quantities
                    if x is not None:
                        assert float((x - y).abs().max()) <= 1e-9 * max(1.0, float(y.abs().max()))
                for _ in range(3):
                    _window_us(kernel, 20)
                    _window_us(base, 20)
                tk, tb = [], []
                for _ in range(args.windows):
                    tk.append(_window_us(kernel, args.calls))
                    tb.append(_window_us(base, args.calls))
                tag = "hessian" if hessian else "no_hessian"
                r[tag] = dict(kernel_us=round(float(np.median(tk)), 2), kernel_spread_us=round(max(tk) - min(tk), 2),
                              torch_us=round(float(np.median(tb)), 2), torch_spread_us=round(max(tb) - min(tb), 2))
            r["pass_gbytes_per_s"] = round(4.0 * n * m / (r["no_hessian"]["kernel_us"] * 1e-6) / 1e9, 1)
            res["%s_observed_%s_percent" % (family, frac)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
