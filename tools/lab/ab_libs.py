"""Lab: wall time per C3 CG solve of TWO BUILDS of the library in one process (the tree's against a parent's built beside it).
Both libraries are loaded by path, as tools/lab/stamp_solve.py loads its stamped build; one plan per library on the same workload,
alternating blocks of solves, so that box-to-box and minute-to-minute drift hits both sides alike (tools/lab/ab_fold.py).  Prints the
median, the extremes and every block mean per side, the gain against the larger max - min spread, and whether the two solutions are
the same bits.
Usage: ab_libs.py <library A (e.g. the parent's)> <library B (default: the tree's)> [blocks] [solves per block] [--keep-first-block]"""
import argparse, ctypes, gc, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
from manifold_gp_amd import _lib


def load(path):
    """ctypes handle with the signatures of _lib.SIGNATURES; a symbol the (older) build does not have yet is left out"""
    h = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return h


paths = [sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else _lib.LIB_PATH]
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 15
per = int(sys.argv[4]) if len(sys.argv) > 4 else 100
libs = [load(p) for p in paths]
_lib._LIB = libs[1]                      # the workload (graph, tiles, Laplacian) is built once, by the second library
import torch
import bench
from manifold_gp_amd.solvers import CgPlan
dev = torch.device("cuda:0")
wl = bench.build_workload(argparse.Namespace(workload="c3", nodes=0, s5_order="morton"), dev, 0, 1)
y = wl["y"].view(-1, 1).contiguous()
plans = []
for h in libs:
    _lib._LIB = h
    plans.append(CgPlan(wl["desc"], 1, tol=1e-6, max_iter=5000, stop_mode=1, check_every=8, refine=0))


def solve(k, **kw):
    _lib._LIB = libs[k]
    return plans[k].solve(y, **kw)


for _ in range(1500):                    # clocks up, graphs captured on both plans
    solve(0, copy=False); solve(1, copy=False)
gc.collect(); gc.disable()
us = [[], []]
# The first block behind the pause above runs 1.2-1.5 us per solve slow for whichever library takes it and 0.5 for the other (seen
# with either library first): one pair of blocks is run and discarded, so that no side carries a cold block the other does not.
# `--keep-first-block` times it as ab_fold.py does.
for b in range(0 if "--keep-first-block" in sys.argv else -1, blocks):
    for k in ((0, 1) if b % 2 == 0 else (1, 0)):
        for _ in range(20):
            solve(k, copy=False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(per):
            solve(k, copy=False)
        torch.cuda.synchronize()
        if b >= 0:
            us[k].append((time.perf_counter() - t0) / per * 1e6)
gc.enable()
sols = []
for k in (0, 1):
    sols.append(solve(k).clone())
    v, p = us[k], plans[k]
    print("%s: median %.2f us per solve, min %.2f max %.2f (spread %.2f) over %d blocks of %d;  folded %d iters %d status %d resid %.6e applies %d"
          % (paths[k], statistics.median(v), min(v), max(v), max(v) - min(v), len(v), per, p.folded, p.iters, p.status, max(p.resid),
             p.applies), flush=True)
    print("   blocks: " + " ".join("%.1f" % t for t in v), flush=True)
gain = statistics.median(us[0]) - statistics.median(us[1])
spread = max(max(v) - min(v) for v in us)
print("gain of the second library %.2f us per solve (medians) = %.1f x the larger spread (%.2f us);  solutions bit-identical: %s"
      % (gain, gain / spread if spread > 0 else float("inf"), spread, bool(torch.equal(sols[0], sols[1]))))
for k in (0, 1):
    _lib._LIB = libs[k]
    plans[k].close()
