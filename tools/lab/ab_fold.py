"""Lab: wall time per C3 CG solve with the vector update folded into the second SpMV of the apply (mgp_cg_set_fold_update 1)
against the (apply, update) launches (0).  One process, one plan per setting, alternating blocks of 100 solves: box-to-box and
minute-to-minute drift hits both sides alike.  Prints the median, the quartiles, the extremes and every block mean per side, and how far the two
solutions are apart.  Usage: ab_fold.py [workload] [blocks] [solves per block]"""
import os, sys, argparse, time, statistics, gc
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
import torch
import bench
from manifold_gp_amd import _lib
from manifold_gp_amd.solvers import CgPlan
dev = torch.device("cuda:0")
wl = bench.build_workload(argparse.Namespace(workload=sys.argv[1] if len(sys.argv) > 1 else "c3", nodes=0, s5_order="morton"), dev, 0, 1)
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 7
per = int(sys.argv[3]) if len(sys.argv) > 3 else 100
y = wl["y"].view(-1, 1).contiguous()
lib = _lib.lib()
plans = {}
for mode in (0, 1):
    prev = lib.mgp_cg_set_fold_update(mode)
    plans[mode] = CgPlan(wl["desc"], 1, tol=1e-6, max_iter=5000, stop_mode=1, check_every=8, refine=0)
    lib.mgp_cg_set_fold_update(prev)
    assert plans[mode].folded == bool(mode)
for _ in range(1500):                       # clocks up, graphs captured on both plans
    plans[0].solve(y, copy=False); plans[1].solve(y, copy=False)
gc.collect(); gc.disable()
us = {0: [], 1: []}
for b in range(blocks):
    for mode in ((0, 1) if b % 2 == 0 else (1, 0)):
        plan = plans[mode]
        for _ in range(20):
            plan.solve(y, copy=False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(per):
            plan.solve(y, copy=False)
        torch.cuda.synchronize()
        us[mode].append((time.perf_counter() - t0) / per * 1e6)
gc.enable()
sols = {}
for mode in (0, 1):
    x = plans[mode].solve(y).clone()
    sols[mode] = x
    v = us[mode]
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    print("fold %d: median %.2f us per solve, quartiles %.2f .. %.2f, min %.2f max %.2f over %d blocks of %d;  iters %d status %d resid %.3e applies %d"
          % (mode, statistics.median(v), q[0], q[2], min(v), max(v), len(v), per, plans[mode].iters, plans[mode].status,
             max(plans[mode].resid), plans[mode].applies), flush=True)
    print("   blocks: " + " ".join("%.1f" % t for t in v), flush=True)
d = float((sols[0] - sols[1]).abs().max() / sols[0].abs().max())
print("gain %.2f us per solve (medians);  max |x_fold - x_unfolded| / max |x| = %.3e" % (statistics.median(us[0]) - statistics.median(us[1]), d))
for p in plans.values():
    p.close()
