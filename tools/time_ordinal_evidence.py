"""Time the two kernels of the ordinal evidence (mgp_ordinal_evidence_site and mgp_ordinal_cut_sums, both launches each) and the
two of the negative-binomial evidence that run the same node loop (mgp_nb_evidence_site, mgp_nb_dispersion_sums; r = 2, counts of
mean 20, a sixth of them above the 32 where the digamma difference changes its form) through the C entry points with preallocated outputs: device events around a window of back-to-back calls on one stream, after 50 warm-up
calls, five windows each, at n = 60 000 and n = 1 000 000 (K = 5, every node observed, var and u given).  The method of the table
in docs/kernels/ordinal.md and of "Learning the dispersion" in docs/kernels/counts.md.  Prints one JSON line.  Nothing here is an acceptance bar.

    python tools/time_ordinal_evidence.py [--calls 2000] [--windows 5]
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


def _windows(call, calls, windows, warmup=50):
    """microseconds per call of every window"""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record()
        b.synchronize()
        out.append(round(a.elapsed_time(b) * 1e3 / calls, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    from manifold_gp_amd import _lib
    from manifold_gp_amd._lib import check, ptr, stream
    lib = _lib.lib()
    assert torch.cuda.is_available(), "this tool needs the MI355X"
    dev = torch.device("cuda:0")
    K = 5
    cuts = np.array([-1.5, -0.5, 0.5, 1.5])
    res = dict(tool="time_ordinal_evidence", K=K, calls=args.calls)
    for n in (60000, 1000000):
        rng = np.random.default_rng(n)
        cat = rng.integers(0, K, n)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        f = up((rng.standard_normal(n) * 2.0).astype(np.float32))
        lo = up(np.concatenate([[-np.inf], cuts])[cat].astype(np.float32))
        hi = up(np.concatenate([cuts, [np.inf]])[cat].astype(np.float32))
        catd, var, u = up(cat.astype(np.uint8)), up(rng.uniform(0.01, 9.0, n)), up(rng.standard_normal(n))
        root, corr = torch.empty_like(f), torch.empty_like(f)
        sums = torch.empty(4, dtype=torch.float64, device=dev)
        out = torch.empty((3, K - 1), dtype=torch.float64, device=dev)
        work = torch.empty(max(lib.mgp_ordinal_evidence_site_workspace_bytes(n), lib.mgp_ordinal_cut_sums_workspace_bytes(n, K)),
                           dtype=torch.uint8, device=dev)
        st = stream()

        def site():
            check(lib.mgp_ordinal_evidence_site(ptr(f), ptr(lo), ptr(hi), None, ptr(var), n, 1e-30, ptr(root), ptr(corr), ptr(sums),
                                                ptr(work), work.numel(), st), "mgp_ordinal_evidence_site")

        def cut_sums():
            check(lib.mgp_ordinal_cut_sums(ptr(f), ptr(lo), ptr(hi), ptr(catd), None, ptr(var), ptr(u), n, K, 1e-30, ptr(out),
                                           ptr(work), work.numel(), st), "mgp_ordinal_cut_sums")
        y = up(rng.negative_binomial(2.0, 2.0 / 22.0, n).astype(np.float32))
        aux = up(np.log(rng.uniform(0.5, 20.0, n)).astype(np.float32))
        out3 = torch.empty(3, dtype=torch.float64, device=dev)

        def nb_site():
            check(lib.mgp_nb_evidence_site(ptr(f), ptr(y), ptr(aux), None, ptr(var), n, 0.0, 2.0, 1e-30, ptr(root), ptr(corr), ptr(sums),
                                           ptr(work), work.numel(), st), "mgp_nb_evidence_site")

        def nb_dispersion():
            check(lib.mgp_nb_dispersion_sums(ptr(f), ptr(y), ptr(aux), None, ptr(var), ptr(u), n, 0.0, 2.0, 1e-30, ptr(out3), ptr(work),
                                             work.numel(), st), "mgp_nb_dispersion_sums")
        res["evidence_site_us_n%d" % n] = _windows(site, args.calls, args.windows)
        res["cut_sums_us_n%d" % n] = _windows(cut_sums, args.calls, args.windows)
        res["nb_evidence_site_us_n%d" % n] = _windows(nb_site, args.calls, args.windows)
        res["nb_dispersion_sums_us_n%d" % n] = _windows(nb_dispersion, args.calls, args.windows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
