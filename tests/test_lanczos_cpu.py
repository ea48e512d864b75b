"""The bounds of the Lanczos invariants (tests/_lanczos_ref.py), fixed and shown to discriminate WITHOUT the code under test.

The float32 numpy restatement of the kernels' algorithm, summed in the kernels' order, runs on k-NN swiss rolls of 9, 67, 20,011
and 525,319 nodes (host k-NN, bandwidth from synth.bandwidth_rule, float64 Laplacian of oracle/laplacian.py, operator of
oracle/sparse.py).  Clean, it must pass I0, I1 and I2; with one planted error it must fail the invariant that error belongs to.

Measured (this file prints every figure; units of u = 2^-24, I2 in u ||A||):
  clean     swiss rolls: I0 <= 2.3 (bounds 8.5 ... 133), I1 <= 5.3 (67 nodes, P = 3), I2 <= 1.4 (67 nodes, P = 16); at 525,319 rows
            1.1 / 2.9 / 0.6.  The rings of the GPU width sweep (every P, n = 2 ... 2,051, every column): I0 <= 0.20 of its bound,
            I1 <= 15.5, I2 <= 3.1 (both at P = 1, 257 nodes)
            -> I1_BOUND = 256, I2_BOUND = 64 (16 times the worst, rounded up to a power of two)
  planted   see test_planted_errors_are_caught
At 525,319 rows a single row is below the bounds (a row is 2e-6 of a dot product): the ragged-edge coverage (skip_last_row,
double_row) comes from the sizes up to 20,011, the dropped-workgroup coverage from every size, the large one included.
"""
import math

import numpy as np
import pytest
import torch

import _lanczos_ref as lr
from oracle.solvers import lanczos_tridiag_f64

U = lr.U
# (name, n, k, nu, kappa / eps, P (None: single-vector form), steps)
CASES = [
    ("20k P12 nu2", 20011, 10, 2, 3.0, 12, 20),
    ("20k P13 nu2 deep", 20011, 10, 2, 3.0, 13, 47),
    ("20k P5 nu1", 20011, 10, 1, 1.0, 5, 47),
    ("20k P16 nu3", 20011, 10, 3, 10.0, 16, 20),
    ("20k single nu2", 20011, 10, 2, 3.0, None, 30),
    ("67 P16", 67, 10, 2, 3.0, 16, 20),
    ("67 P3", 67, 10, 2, 3.0, 3, 20),
    ("67 single", 67, 10, 2, 3.0, None, 20),
    ("9 P16", 9, 4, 2, 3.0, 16, 5),
    ("9 P1", 9, 4, 2, 3.0, 1, 5),
    ("525k P16", 525319, 10, 2, 3.0, 16, 12),
]
SCALE = 0.7
_GRAPHS = {}


def _setup(case):
    name, n, k, nu, kmult, P, steps = case
    if (n, k) not in _GRAPHS:
        _GRAPHS[(n, k)] = lr.swiss_graph(n, k, seed=3)
    idx, val, eps = _GRAPHS[(n, k)]
    Pm, matmul32, normA = lr.host_operator(idx, val, n, eps, nu, kmult * eps, SCALE)
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((n, 2)).astype(np.float32) * np.array([1.0, 2.0 ** -5], np.float32)
    return Pm, matmul32, normA, Z


def _figures(case, plant=None):
    name, n, k, nu, kmult, P, steps = case
    Pm, matmul32, normA, Z = _setup(case)
    al, be, Q = lr.lanczos_f32(matmul32, Z[:, 0], steps, P, plant, z_other=Z[:, 1])
    mm = lambda V: torch.from_numpy(Pm.matmul(V.numpy()))       # noqa: E731
    return lr.invariants(torch.from_numpy(Z[:, 0]), al, be, torch.from_numpy(Q), mm, normA)


def _ring_figures():
    """The width sweep of tests/test_gpu_lanczos.py (every P, every ring, every column) through the restatement: the worst
    (I0 / its bound, I1, I2) and where."""
    worst, where = [0.0, 0.0, 0.0], [None, None, None]
    for P in range(1, 17):
        for c in lr.ring_cases(P):
            assert c["steps"] <= c["n"] - 1 and c["min_beta"] >= lr.PRECONDITION * c["normA"]
            mm = lambda V: torch.from_numpy(c["Pm"].matmul(V.numpy()))       # noqa: E731
            L = lr.blz_chain(c["n"], P)
            for p in range(P):
                al, be, Q = lr.lanczos_f32(c["matmul32"], c["Z"][:, p], c["steps"], P)
                i0, i1, i2 = lr.invariants(torch.from_numpy(c["Z"][:, p]), al, be, torch.from_numpy(Q), mm, c["normA"])
                for k, v in enumerate((i0 / lr.i0_bound(L), i1, i2)):
                    if v > worst[k]:
                        worst[k], where[k] = v, (P, c["n"], p)
    print("clean rings: I0 %.2f of its bound %s  I1 %.2f %s  I2 %.2f %s" % (worst[0], where[0], worst[1], where[1], worst[2], where[2]))
    return tuple(worst)


@pytest.fixture(scope="module")
def clean():
    out = {}
    for case in CASES:
        out[case[0]] = _figures(case)
        name, n, k, nu, kmult, P, steps = case
        L = lr.lz_chain(n) if P is None else lr.blz_chain(n, P)
        print("clean %-18s chain %4d  I0 %.2f (bound %.1f)  I1 %.2f  I2 %.2f" % ((name, L) + out[name][:1] + (lr.i0_bound(L),)
                                                                                 + out[name][1:]))
        out[name] = (out[name][0] / lr.i0_bound(L),) + out[name][1:]
    out["rings"] = _ring_figures()
    return out


def test_geometry_reproduces_the_constants_of_eigen_hip():
    """blz_layout (csrc/eigen.hip:1040-1045): 256 workgroups at most, 4 RL rows each at least, element grids of 2048 at most;
    mgp_lanczos_tridiag (:1206-1210): 512 workgroups of 1024 rows; kBlzMaxNq = 48, kBlzMaxP = 16 (:865-866); the reduce loop's
    `b0 += 32` (:926)."""
    for P in range(1, 17):
        RL = 256 // P
        assert lr.blz_geometry(4 * RL, P)[:3] == (RL, 1, 4 * RL)
        assert lr.blz_geometry(4 * RL + 1, P)[1] == 2
        assert lr.blz_geometry(256 * 4 * RL, P)[1:3] == (256, 4 * RL)
        RLg, nblk, rpb, egrid = lr.blz_geometry(256 * 4 * RL + 1, P)
        assert nblk <= 256 and rpb == 4 * RL + 1 and nblk * rpb >= 256 * 4 * RL + 1
        assert lr.blz_geometry(2048 * 256 // P + 300, P)[3] == 2048 and lr.blz_geometry(2047 * 256 // P, P)[3] <= 2047
    assert lr.blz_geometry(525319, 16) == (16, 256, 2053, 2048)
    assert lr.blz_geometry(525319, 1) == (256, 256, 2053, 2048)          # (ceil(525319 / 256) = 2053 > 2048)
    assert lr.blz_reduce_trips(256) == 8 and lr.blz_reduce_trips(32) == 1 and lr.blz_reduce_trips(33) == 2
    assert lr.lz_geometry(1546) == (2, 773, 7)
    assert lr.lz_geometry(512 * 1024) == (512, 1024, 2048)
    assert lr.lz_geometry(525319) == (512, 1027, 2048) and 525319 > 512 * 1024
    assert lr.lz_geometry(1) == (1, 1, 1) and lr.blz_geometry(1, 16) == (16, 1, 1, 1)
    assert lr.blz_dots_lds_bytes(16, 48) == 48 * 1024 and lr.blz_dots_lds_bytes(13, 48) == 48 * 19 * 13 * 4
    # the graph every older Lanczos test runs on: 13 workgroups at most, one trip of the reduce loop
    assert max(lr.blz_geometry(1546, P)[1] for P in (4, 8, 12, 16)) <= 32
    assert lr.blz_chain(525319, 16) == 129 + 16 + 64 + 2 and lr.lz_chain(525319) == 5 + 9 + 512


def test_summation_order_is_the_sum():
    """The restated summation adds every row exactly once (integers: exact in any order)."""
    rng = np.random.default_rng(0)
    for n, P in ((9, 16), (67, 3), (20011, 13), (20011, None), (70001, 1)):
        v = rng.integers(-8, 9, (3, n)).astype(np.float32)
        S = lr.Summation(n, P)
        assert np.array_equal(S.total(S.partials(v)), v.sum(1, dtype=np.float64).astype(np.float32)), (n, P)


def test_preconditions_hold_in_float64():
    """min_j beta_j >= 2^-6 normA on the float64 run of every case, and steps <= n - 1."""
    for case in CASES:
        name, n, k, nu, kmult, P, steps = case
        Pm, _, normA, Z = _setup(case)
        assert steps <= n - 1
        a, b = lanczos_tridiag_f64(Pm.matmul, Z[:, 0].astype(np.float64), steps + 1)
        assert len(b) == steps, name
        print("%-18s min beta / normA = 2^%.2f" % (name, math.log2(b.min() / normA)))
        assert b.min() >= lr.PRECONDITION * normA, (name, b.min() / normA)


def test_clean_restatement_is_inside_the_bounds(clean):
    for name, (r0, i1, i2) in clean.items():
        assert r0 <= 1.0, (name, r0)
        assert i1 <= lr.I1_BOUND and i2 <= lr.I2_BOUND, (name, i1, i2)


def test_bounds_are_sixteen_times_the_restatement(clean):
    """I1_BOUND, I2_BOUND = 16 x the worst clean figure, rounded up to a power of two."""
    w1 = max(v[1] for v in clean.values())
    w2 = max(v[2] for v in clean.values())
    print("worst clean I1 %.3f u, I2 %.3f u||A||" % (w1, w2))
    assert lr.I1_BOUND == 2 ** math.ceil(math.log2(16 * w1)), w1
    assert lr.I2_BOUND == 2 ** math.ceil(math.log2(16 * w2)), w2
    assert abs(w1 - lr.I1_MEASURED) < 0.06 and abs(w2 - lr.I2_MEASURED) < 0.06


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planted_errors_are_caught(case):
    """drop_block fails I1 and I2 at every size; skip_last_row and double_row fail I2 up to 20,011 rows; swap_columns fails I0 and
    nothing else.  Measured (I1 in u / I2 in u ||A||; bounds 256 / 64):
      drop_block      525,319 rows: 72,300 / 1,050;  20,011: 79,700 ... 938,000 / 2,600 ... 26,500;  67 (two workgroups): 1e9 / 2e7
      skip_last_row,  20,011 rows, nu = 1 and 2: 1,260 ... 3,030 / 150 ... 335;  67 and 9 rows: 1e6 ... 3e7 / 2e5 ... 6e5
      double_row
      swap_columns    I0 = 2.2e7 ... 2.4e7 u (bounds 8.5 ... 133), I1 <= 5.4, I2 <= 1.3
    Where the geometry has ONE workgroup (9 rows; 67 rows at P = 3 and in the single-vector form) dropping it leaves nothing: the
    figures are not finite, which counts as a failure.  At nu = 3 the Gershgorin bound of ||A|| cubes its slack and a single row of
    20,011 moves I2 to 20 u ||A|| only, under the bound: the single-row errors are asserted at nu = 1 and 2 (what the GPU tests
    run), the nu = 3 case keeps the clean run and the dropped workgroup."""
    name, n, k, nu, kmult, P, steps = case
    L = lr.lz_chain(n) if P is None else lr.blz_chain(n, P)
    i0, i1, i2 = _figures(case, "drop_block")
    print("%-18s drop_block     I1 %.3g  I2 %.3g" % (name, i1, i2))
    assert i1 > lr.I1_BOUND and i2 > lr.I2_BOUND, (name, i1, i2)
    if n <= 20011 and nu <= 2:
        for plant in ("skip_last_row", "double_row"):
            i0, i1, i2 = _figures(case, plant)
            print("%-18s %-14s I1 %.3g  I2 %.3g" % (name, plant, i1, i2))
            assert i2 > lr.I2_BOUND, (name, plant, i2)
    i0, i1, i2 = _figures(case, "swap_columns")
    print("%-18s swap_columns   I0 %.3g  I1 %.3g  I2 %.3g" % (name, i0, i1, i2))
    assert i0 > lr.i0_bound(L) and i0 > 1e5, (name, i0)
    assert i1 <= lr.I1_BOUND and i2 <= lr.I2_BOUND, "a wrong start vector is invisible to I1 and I2"
