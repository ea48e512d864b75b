"""The 300,071-node swiss roll that the past-the-caps tests share (tests/test_gpu_past_caps.py, tests/test_gpu_solver_contract.py).

n = 300,071 is just beyond every size cap of the forward SpMM and the CG kernels (csrc/spmm_policy.h kMaxGrid = 4096 workgroups,
csrc/cg.hip 2 x 32 x TS delta partials per round trip): ceil(n / 64) = 4689 row tiles (two tiles per workgroup, the last
workgroup holds one), n % 64 = 39 and n % 16 = 7 (ragged last tiles).  Built as `swiss150k` of tests/test_gpu_gradients.py
is: k = 10, the bandwidth from synth.bandwidth_rule on the nearest-neighbour distances.  Each module that uses it builds the graphs
in a module-scoped fixture of its own (k-NN, graph, tiles: 0.4 s for both row orders on the MI355X) and lets them go with it."""
import time

import numpy as np
import torch

N = 300_071
K = 10
MAX_GRID = 4096            # csrc/spmm_policy.h kMaxGrid
BLOCK = 256                # csrc/spmm.hip, csrc/cg.hip kBlock


def swiss300k(mgp, dev, order):
    """order "morton": points handed over along a Z-curve (tiles in natural row order); "random": generation order (the tile
    builder picks a locality order: tiles["rowid"]).  Returns dict(knn, graph, idx, val, eps, y, seconds)."""
    from tools import synth
    t0 = time.time()
    x_np, y_np = synth.swiss_roll(N, order=order)
    x = torch.from_numpy(np.ascontiguousarray(x_np)).to(dev)
    knn = mgp.utils.NearestNeighbors(x)
    D, _ = knn.search(x, K)
    idx, val = knn.graph(K)
    eps = synth.bandwidth_rule(D[:, 1].cpu().numpy(), 0.0)[0]
    torch.cuda.synchronize()
    out = dict(knn=knn, graph=knn.knn_graph, idx=idx, val=val, eps=eps, y=y_np, seconds=time.time() - t0)
    print("swiss300k %s: built in %.1f s, M = %d, eps = %.4g" % (order, out["seconds"], knn.knn_graph.M, eps))
    return out


def rows_per_pass(C, lanes):
    """csrc/spmm.hip spmm_rows_per_pass: rows one pass of a gather workgroup covers (C == 1: row groups of `lanes` lanes, one
    row in flight)."""
    if C == 1:
        return BLOCK // lanes
    if C <= 16 and C % 4 == 0:
        return 64
    g = 4
    while g < C and g < 64:
        g <<= 1
    return BLOCK // g * 4


def gather_plan(n, rpp):
    """csrc/spmm.hip make_plan: (grid, rows per workgroup): a whole number of passes, at most MAX_GRID workgroups."""
    grid, rpb = -(-n // rpp), rpp
    if grid > MAX_GRID:
        rpb = -(-(-(-n // MAX_GRID)) // rpp) * rpp
        grid = -(-n // rpb)
    return grid, rpb
