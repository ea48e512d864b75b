"""Lab: wall time per C3 CG solve on the entry-balanced tile set of the single-column tile kernels (graph.C1_BALANCED on) against
the fixed 64-row tiles (off).  One process, one plan per setting, one pair of blocks discarded, then alternating blocks of 100
solves: box-to-box and minute-to-minute drift hits both sides alike.  Prints the tile statistics of both sets, the median, the
quartiles, the extremes and every block mean per side, and how far the two solutions are apart.
Usage: ab_tiles.py [workload] [blocks] [solves per block]"""
import os, sys, argparse, time, statistics, gc, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
import torch
import bench
from manifold_gp_amd import _lib, graph as G
from manifold_gp_amd.solvers import CgPlan
dev = torch.device("cuda:0")
wl = bench.build_workload(argparse.Namespace(workload=sys.argv[1] if len(sys.argv) > 1 else "c3", nodes=0, s5_order="morton"), dev, 0, 1)
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 15
per = int(sys.argv[3]) if len(sys.argv) > 3 else 100
y = wl["y"].view(-1, 1).contiguous()
lib = _lib.lib()
g = wl["graph"]
t = g.tiles
assert t is not None and t.get("c1") is not None, "the policy built no balanced set on this graph (graph.c1_balanced_policy)"


def dist(name, entries, cols):
    e, c = entries.double(), cols.double()
    q = lambda v, p: float(torch.quantile(v, p))
    print("%s: %d tiles; padded entries min %d median %d p90 %d max %d, over %d: %d (over 5120: %d, over 6144: %d); dictionary mean %.0f "
          "p90 %.0f max %d (over 1024: %d), sum %d" % (name, e.numel(), int(e.min()), q(e, 0.5), q(e, 0.9), int(e.max()), G.C1_TILE_CAP,
                                                       int((e > G.C1_TILE_CAP).sum()), int((e > 5120).sum()), int((e > 6144).sum()),
                                                       float(c.mean()), q(c, 0.9), int(c.max()), int((c > 1024).sum()), int(c.sum())), flush=True)


rp = g.rowptr.cpu().long()
edges = rp[torch.clamp(torch.arange(-(-g.n // 64) + 1) * 64, max=g.n)]
tp = t["tile_ptr"].cpu().long()
dist("64-row tiles", edges[1:] - edges[:-1], tp[1:] - tp[:-1])
c1 = t["c1"]
first, tp1 = c1["first"], c1["tile_ptr"].cpu().long()
dist("balanced tiles", rp[first[1:]] - rp[first[:-1]], tp1[1:] - tp1[:-1])
h = first[1:] - first[:-1]
print("balanced heights: min %d, under 64 rows: %d" % (int(h.min()), int((h < 64).sum())), flush=True)

plans = {}
for mode in (0, 1):
    G.C1_BALANCED[0] = bool(mode)
    plans[mode] = CgPlan(wl["desc"], 1, tol=1e-6, max_iter=5000, stop_mode=1, check_every=8, refine=0)
    nbs = lib.mgp_spmm_dot_blocks_csr(ctypes.byref(plans[mode].op.L), 1)
    assert nbs == (c1["T"] if mode else -(-g.n // 64)), (mode, nbs)
    print("balanced %d: %d SpMV workgroups, folded %s" % (mode, nbs, plans[mode].folded), flush=True)
G.C1_BALANCED[0] = True
for _ in range(1500):                       # clocks up, graphs captured on both plans
    plans[0].solve(y, copy=False); plans[1].solve(y, copy=False)
gc.collect(); gc.disable()
us = {0: [], 1: []}
for b in range(-1, blocks):                 # (block -1: one pair discarded)
    for mode in ((0, 1) if b % 2 == 0 else (1, 0)):
        plan = plans[mode]
        for _ in range(20):
            plan.solve(y, copy=False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(per):
            plan.solve(y, copy=False)
        torch.cuda.synchronize()
        if b >= 0:
            us[mode].append((time.perf_counter() - t0) / per * 1e6)
gc.enable()
sols = {}
for mode in (0, 1):
    x = plans[mode].solve(y).clone()
    sols[mode] = x
    v = us[mode]
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    print("balanced %d: median %.2f us per solve, quartiles %.2f .. %.2f, min %.2f max %.2f (spread %.2f) over %d blocks of %d;  iters %d status %d "
          "resid %.3e applies %d" % (mode, statistics.median(v), q[0], q[2], min(v), max(v), max(v) - min(v), len(v), per, plans[mode].iters,
                                     plans[mode].status, max(plans[mode].resid), plans[mode].applies), flush=True)
    print("   blocks: " + " ".join("%.1f" % t for t in v), flush=True)
d = float((sols[0] - sols[1]).abs().max() / sols[0].abs().max())
gain = statistics.median(us[0]) - statistics.median(us[1])
spread = max(max(v) - min(v) for v in us.values())
print("gain %.2f us per solve (medians), %.1f x the larger max - min spread (%.2f);  max |x_balanced - x_64| / max |x| = %.3e"
      % (gain, gain / spread if spread > 0 else float("inf"), spread, d))
for p in plans.values():
    p.close()
