"""The entry-balanced row tiles of the single-column tile kernels: the cut, its padded position space and the policy (no GPU).

graph.c1_balanced_cut is a greedy pass over the rows in their natural order: a tile ends at 64 rows or when the next row would take
it past C1_TILE_CAP padded entries; one row heavier than the cap is a tile of its own.  c1_padded_positions lays the tiles out in
positions 64 t .. 64 t + 63 (rows first, then empty positions) and c1_balanced_policy says when the set is built at all
(docs/kernels/spmm.md, round 8)."""
import os
import re

import pytest
import torch

from manifold_gp_amd import graph as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = G.C1_TILE_CAP


def rowptr_of(lengths):
    rp = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.as_tensor(lengths, dtype=torch.int64), 0)
    return rp


def lengths_case(name):
    g = torch.Generator().manual_seed(7)
    quads = lambda n, lo, hi: (4 * torch.randint(lo, hi, (n,), generator=g)).tolist()
    if name.startswith("n"):                       # n1, n63, n64, n65, n1000: rows of 13 to 44 quads (52 to 176 entries, the k-NN range)
        return quads(int(name[1:]), 13, 45)
    if name == "empty":
        return [0] * 200
    if name == "hub":                              # one row over the cap among light rows
        l = quads(300, 1, 6)
        l[137] = CAP + 904
        return l
    if name == "hub_first":
        return [CAP + 4] + quads(70, 1, 6)
    if name == "hub_last":
        return quads(70, 1, 6) + [CAP + 4]
    if name == "heavy":                            # every row over the cap
        return [CAP + 4 * i for i in range(1, 80)]
    if name == "exact":                            # rows that fill a tile to the cap exactly: 16 rows of 256 entries
        return [256] * 100
    raise KeyError(name)


CASES = ["n1", "n63", "n64", "n65", "n1000", "empty", "hub", "hub_first", "hub_last", "heavy", "exact"]


@pytest.mark.parametrize("name", CASES)
def test_cut(name):
    lengths = lengths_case(name)
    rp, n = rowptr_of(lengths), len(lengths)
    first = G.c1_balanced_cut(rp)
    T = first.numel() - 1
    assert first[0] == 0 and first[-1] == n                          # the tiles cover 0 .. n in order
    h = first[1:] - first[:-1]
    assert int(h.min()) >= 1 and int(h.max()) <= 64
    e = rp[first[1:]] - rp[first[:-1]]
    assert bool(((e <= CAP) | (h == 1)).all())                        # over the cap: a single row only
    for t in range(T - 1):                                           # greedy-maximal: the next row would break a limit
        nxt = int(first[t + 1])
        assert int(h[t]) == 64 or int(e[t]) + lengths[nxt] > CAP, (t, int(h[t]), int(e[t]), lengths[nxt])
    if name == "exact":
        assert bool((e[:-1] == CAP).all()) and bool((h[:-1] == 16).all())
    if name == "heavy":
        assert T == n
    if name == "empty":
        assert T == -(-n // 64)


@pytest.mark.parametrize("name", CASES)
def test_padded_positions(name):
    lengths = lengths_case(name)
    rp, n = rowptr_of(lengths), len(lengths)
    first = G.c1_balanced_cut(rp)
    T = first.numel() - 1
    pad, shift = G.c1_padded_positions(rp, first)
    assert pad.numel() == 64 * T + 1 and shift.numel() == T + 1
    assert pad[0] == 0 and pad[-1] == rp[-1] and bool((pad[1:] >= pad[:-1]).all())
    assert shift[T] == 64 * T - n
    for t in range(T):
        f, h = int(first[t]), int(first[t + 1] - first[t])
        assert int(shift[t]) == 64 * t - f                           # position p of tile t is row p - shift[t]
        assert h == 64 - int(shift[t + 1] - shift[t])                # the height, as the kernel takes it
        assert torch.equal(pad[64 * t:64 * t + h + 1], rp[f:f + h + 1])      # the rows first, with their own extents
        assert bool((pad[64 * t + h:64 * t + 65] == rp[f + h]).all())        # then empty positions


def test_cap_is_the_kernels():
    """The cap is what a workgroup holds in registers, 4 entries x NQ quads x BS lanes: stated in the header, asserted against the
    kernel's constants in the source, mirrored in graph.py."""
    header = open(os.path.join(ROOT, "include", "mgp_hip.h")).read()
    src = open(os.path.join(ROOT, "manifold_gp_amd", "csrc", "spmm.hip")).read()
    cap = int(re.search(r"#define\s+MGP_C1_TILE_CAP\s+(\d+)", header).group(1))
    assert cap == CAP
    body = src[src.index("void spmv_tile_body("):src.index("void spmv_tile_kernel(")]
    assert re.search(r"static_assert\(BS != 256 \|\| 4 \* NQ \* BS == MGP_C1_TILE_CAP", body)
    nq = int(re.search(r"constexpr int NQ = (\d+);", body).group(1))
    assert 4 * nq * 256 == CAP                                       # BS = 256: the 64-row tiles' workgroup
    policy = open(os.path.join(ROOT, "manifold_gp_amd", "csrc", "spmm_policy.h")).read()      # the constants the kernels share with the plan
    assert '#include "spmm_policy.h"' in src and "kMaxGrid =" not in src
    assert G.C1_MAX_TILES == int(re.search(r"constexpr int kMaxGrid = (\d+);", policy).group(1))


def test_policy_no_heavy_tile():
    assert G.c1_balanced_policy(rowptr_of([60] * 1000)) is None      # 64 rows of 60: 3840 entries a tile
    assert G.c1_balanced_policy(rowptr_of([64] * 1000)) is None      # exactly at the cap: nothing loops
    assert G.c1_balanced_policy(rowptr_of([0] * 10)) is None
    first = G.c1_balanced_policy(rowptr_of([68] + [64] * 999))       # one tile over it
    assert first is not None and first[-1] == 1000


def test_policy_keeps_the_folded_step():
    """60 000 rows, 938 fixed tiles: a cut that lands over 1024 tiles would take the plan's four-slot folded step away."""
    n = 60000
    assert -(-n // 64) == 938
    rp = rowptr_of([72] * n)                                         # 56 rows fill the cap: 1072 tiles
    assert G.c1_balanced_cut(rp).numel() - 1 == 1072
    assert G.c1_balanced_policy(rp) is None
    g = torch.Generator().manual_seed(3)
    lengths = (4 * torch.randint(13, 19, (n,), generator=g)).tolist()      # mean 62 entries: heavy tiles, yet under 1024
    first = G.c1_balanced_policy(rowptr_of(lengths))
    assert first is not None and 938 <= first.numel() - 1 <= 1024


def test_policy_orders_and_sizes():
    rp = rowptr_of([72] * 2000)
    assert G.c1_balanced_policy(rp) is not None
    assert G.c1_balanced_policy(rp, ordered=True) is None            # a row order present: the 64-row set alone
    assert G.c1_balanced_policy(rp, rows=32) is None
    assert G.c1_balanced_policy(rowptr_of([72] * (64 * 4096 + 1))) is None       # the loop form
    assert G.c1_balanced_policy(rowptr_of([72] * (56 * 4096 + 1))) is None       # the balanced set past 4096 tiles


def test_switch_is_one_cell():
    from manifold_gp_amd import _lib
    assert G.C1_BALANCED is _lib.C1_BALANCED and G.C1_BALANCED == [True]
