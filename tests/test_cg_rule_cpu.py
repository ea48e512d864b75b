"""The CG step rule (manifold_gp_amd/csrc/cg_rule.h) on the CPU: the header compiles with a host compiler alone, so a small C++
probe runs the Chronopoulos-Gear recurrence in float on an 8 x 8 SPD system and takes EVERY coefficient and decision from the
header -- the same functions the update / decide kernels of cg.hip and pcg.hip call.

The oracle is numpy.linalg.solve in float64 and the contract written at the top of tests/test_gpu_solver_contract.py (C1, C2,
C4, C5 and its fp32 floor F = 4 eps32 ||A||_2 ||x|| / ||b||), never a transliteration of the rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
EPS32 = float(np.finfo(np.float32).eps)
N = 8

PROBE = r"""
#include <stdio.h>
#include "cg_rule.h"
enum { N = 8 };
static float dot(const float* a, const float* b) { float t = 0.f; for (int i = 0; i < N; ++i) t += a[i] * b[i]; return t; }
int main(void) {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'c') {          // coefficients alone: first frozen gamma delta gamma_old alpha_old
      int first, frozen; float g, d, go, ao;
      if (scanf("%d %d %f %f %f %f", &first, &frozen, &g, &d, &go, &ao) != 6) return 1;
      const CgCoef k = cg_coef(first != 0, frozen != 0, g, d, go, ao);
      printf("%.9g %.9g\n", k.alpha, k.beta);
      continue;
    }
    // a solve: stop_mode min_iter max_iter tol zero_based, A (row major), b
    int stop_mode, min_iter, max_iter, zero_based; float tol, A[N][N], b[N];
    if (scanf("%d %d %d %f %d", &stop_mode, &min_iter, &max_iter, &tol, &zero_based) != 5) return 1;
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) if (scanf("%f", &A[i][j]) != 1) return 1;
    for (int i = 0; i < N; ++i) if (scanf("%f", &b[i]) != 1) return 1;
    float x[N] = {0}, p[N] = {0}, s[N] = {0}, r[N], w[N];
    for (int i = 0; i < N; ++i) r[i] = b[i];
    float gamma_old = 0.f, alpha_old = 0.f, bb = 0.f, rel = 0.f;
    CgCoef k = {0.f, 0.f};
    CgStop st = {0, 0};
    int steps = 0;             // completed steps: the update of step k decides on r_{k-1}
    for (;; ++steps) {
      for (int i = 0; i < N; ++i) w[i] = dot(A[i], r);                 // u = r: no preconditioner
      const float gamma = dot(r, r), delta = dot(r, w);
      if (steps == 0) bb = gamma;
      rel = cg_rel(gamma, bb);
      // cg.hip counts the deciding update from 1, pcg.hip from 0 and passes it + 1
      if (zero_based) { const int it = steps; st = cg_stop(stop_mode, min_iter, max_iter, tol, it + 1, rel); }
      else { const int it = steps + 1; st = cg_stop(stop_mode, min_iter, max_iter, tol, it, rel); }
      k = cg_coef(steps == 0, cg_frozen(stop_mode, tol, rel), gamma, delta, gamma_old, alpha_old);
      if (st.done) break;
      for (int i = 0; i < N; ++i) {
        p[i] = k.beta * p[i] + r[i];
        s[i] = k.beta * s[i] + w[i];
        x[i] += k.alpha * p[i];
        r[i] -= k.alpha * s[i];
      }
      gamma_old = gamma; alpha_old = k.alpha;
    }
    for (int i = 0; i < N; ++i) printf("%.9g ", x[i]);
    printf("%d %d %.9g %.9g %.9g\n", steps, st.status, rel, k.alpha, k.beta);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("cg_rule")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([CXX, "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.check_output([str(exe)], input="\n".join(lines) + "\n", text=True)
        return [[float(v) for v in ln.split()] for ln in out.strip().splitlines()]
    return run


def spd(eigs, seed=0):
    """A = Q diag(eigs) Q^T, rounded to float32 (the matrix the probe sees), and a right-hand side with weight on every mode."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    A = (Q * np.asarray(eigs, np.float64)) @ Q.T
    A = (0.5 * (A + A.T)).astype(np.float32)
    b = (Q @ rng.uniform(0.5, 1.5, N)).astype(np.float32)
    return A, b


def solve_line(A, b, stop_mode, min_iter, max_iter, tol, zero_based=0):
    return "s %d %d %d %.9g %d " % (stop_mode, min_iter, max_iter, tol, zero_based) + \
        " ".join("%.9g" % v for v in np.concatenate([A.ravel(), b]))


def unpack(row):
    return np.array(row[:N]), int(row[N]), int(row[N + 1]), row[N + 2], row[N + 3], row[N + 4]


def true_rel_and_floor(A, b, x):
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    true_rel = np.linalg.norm(b64 - A64 @ x) / np.linalg.norm(b64)
    F = 4 * EPS32 * np.linalg.norm(A64, 2) * np.linalg.norm(x) / np.linalg.norm(b64)
    return true_rel, F


def test_cg_rule_on_the_host(probe):
    A, b = spd(np.linspace(1.0, 4.0, N))
    A3, b3 = spd([1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0], seed=1)      # three eigenvalues: CG is through in three steps
    bz = np.zeros(N, np.float32)
    bn = b.copy()
    bn[3] = np.nan
    tol = 1e-5
    rows = probe([
        solve_line(A, b, 1, 0, 100, tol),                 # 0 converged, stop_mode 1
        solve_line(A3, b3, 0, 10, 100, 1e-3),             # 1 stop_mode 0, min_iter 10
        solve_line(A, b, 1, 0, 3, 1e-12),                 # 2 max_iter 3, counted from 1 (cg.hip)
        solve_line(A, b, 1, 0, 3, 1e-12, zero_based=1),   # 3 max_iter 3, counted from 0 and passed as it + 1 (pcg.hip)
        solve_line(A, bz, 1, 0, 100, tol),                # 4 zero right-hand side
        solve_line(A, bz, 0, 10, 100, tol),               # 5 the same, linear_cg's rule
        solve_line(A, bn, 1, 0, 100, tol),                # 6 NaN in the right-hand side
        solve_line(A, bn, 0, 10, 100, tol),               # 7
        "c 1 0 2 0 0 0",                                  # 8 delta == 0, first step
        "c 0 0 2 3 0 0.5",                                # 9 gamma_old == 0
        "c 0 0 2 3 4 0",                                  # 10 alpha_old == 0
        "c 0 0 2 2 4 0.5",                                # 11 den = delta - beta gamma / alpha_old == 0
        "c 0 1 2 3 4 0.5",                                # 12 frozen
        "c 0 0 2 3 4 0.5",                                # 13 the plain step
    ])
    # C1: converged in stop_mode 1 -> the TRUE relative residual of the fp32 iterate is within 2 tol + F; F <= tol / 4: not vacuous
    x, steps, status, rel, _, _ = unpack(rows[0])
    x_ref = np.linalg.solve(A.astype(np.float64), b.astype(np.float64))
    true_rel, F = true_rel_and_floor(A, b, x)
    assert status == 1 and 1 <= steps <= N + 2, (status, steps)
    assert F <= tol / 4 and true_rel <= 2 * tol + F, (true_rel, F)
    assert rel <= tol
    assert np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref) <= 2 * np.linalg.cond(A.astype(np.float64)) * true_rel + 1e-5
    # C2: stop_mode 0 runs at least min(10, n - 1) steps although the system is solved after three
    x, steps, status, rel, _, _ = unpack(rows[1])
    true_rel, F = true_rel_and_floor(A3, b3, x)
    assert status == 1 and steps >= min(10, N - 1), (status, steps)
    assert F <= 1e-3 / 4 and true_rel <= 2 * 1e-3 + F, (true_rel, F)
    # C4: max_iter exit: status 2 after exactly max_iter steps, whichever way the deciding update is counted
    for row in (rows[2], rows[3]):
        x, steps, status, rel, _, _ = unpack(row)
        assert status == 2 and steps == 3, (status, steps)
    assert rows[2] == rows[3]
    # C5: a zero right-hand side ends at the first decision with x == 0 exactly, residual 0 and no step taken
    x, steps, status, rel, alpha, beta = unpack(rows[4])
    assert status == 1 and steps == 0 and rel == 0.0 and alpha == 0.0 and beta == 0.0 and not x.any(), rows[4]
    x, steps, status, rel, alpha, beta = unpack(rows[5])
    assert status == 1 and rel == 0.0 and alpha == 0.0 and beta == 0.0 and not x.any(), rows[5]
    # a NaN in the right-hand side is reported, not "converged"
    for row in (rows[6], rows[7]):
        assert int(row[N + 1]) == 3, row
    # the zero-denominator guards: finite coefficients, zero where the guard applies
    assert rows[8] == [0.0, 0.0]
    two_thirds = np.float32(2) / np.float32(3)
    assert np.float32(rows[9][0]) == two_thirds and rows[9][1] == 0.0        # beta = 0: alpha = gamma / delta
    assert np.float32(rows[10][0]) == two_thirds and rows[10][1] == 0.5      # no correction term
    assert rows[11] == [0.0, 0.5]                                            # den == 0: alpha = 0, beta stays
    assert rows[12] == [0.0, 0.0]
    assert rows[13] == [2.0, 0.5]                                            # beta = 2 / 4, alpha = 2 / (3 - 0.5 * 2 / 0.5)
    assert all(np.isfinite(v) for r in rows[8:] for v in r)
