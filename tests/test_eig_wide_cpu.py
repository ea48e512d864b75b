"""Blocks of more than 256 columns on the CPU: the host eigensolver at the sizes such a block hands it (n = 256, 384, 512) against
LAPACK, and the whole Chebyshev-filtered block iteration at b = 384 on a dense 640 x 640 matrix, run by a host-compiled probe
that takes every decision from eig_policy.h (the chunk rule of the block products included) and every Rayleigh-Ritz step from
eig_host.h -- the functions the driver in eigen.hip calls.  The probe is the one of tests/test_eig_policy_cpu.py with the filter
run in the column chunks of eig_chunk_start and a row-parallel mat-vec (a 640 x 640 x 384 product per filter step).

The oracle is numpy in float64 on the matrix the probe sees and the residual theorem for symmetric matrices, as there."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
EPS32 = float(np.finfo(np.float32).eps)
N, M, B = 640, 300, 384
CONVERGED = 1

PROBE = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "eig_host.h"
#include "eig_policy.h"

static uint64_t g_rng;
static float uni() { g_rng = g_rng * 6364136223846793005ULL + 1442695040888963407ULL; return (float)((g_rng >> 40) * (2.0 / 16777216.0) - 1.0); }
static bool rd(double* v) { return scanf("%lf", v) == 1; }
static bool rdi(int* v) { return scanf("%d", v) == 1; }

// Y[:, j] = ca X[:, j] + cb (A X)[:, j] (+ cc Z[:, j]) in float, on `w` columns; rows are independent jobs
static void apply(HostPool& pool, int n, int w, const std::vector<float>& A, const float* X, float* Y, float ca, float cb, const float* Z,
                  float cc) {
  pool.rows(n, 16, [&](int i) {
    std::vector<float> t(w, 0.f);
    for (int k = 0; k < n; ++k) {
      const float a = A[(size_t)i * n + k];
      const float* x = X + (size_t)k * w;
      for (int j = 0; j < w; ++j) t[j] += a * x[j];
    }
    for (int j = 0; j < w; ++j) Y[(size_t)i * w + j] = ca * X[(size_t)i * w + j] + cb * t[j] + (Z ? cc * Z[(size_t)i * w + j] : 0.f);
  });
}

// solve: n b m tol ub ubf tiles max_rounds, A [n x n]
static int solve() {
  int n, b, m, tiles, max_rounds; double tol, ub, ubf, v;
  if (!rdi(&n) || !rdi(&b) || !rdi(&m) || !rd(&tol) || !rd(&ub) || !rd(&ubf) || !rdi(&tiles) || !rdi(&max_rounds)) return 1;
  if (b > kEigMaxBlock) return 1;
  std::vector<float> A((size_t)n * n), V((size_t)n * b), LV((size_t)n * b), Vn((size_t)n * b), LVn((size_t)n * b);
  for (auto& x : A) { if (!rd(&v)) return 1; x = (float)v; }
  g_rng = 1337;
  for (auto& x : V) x = uni();
  EigPolicy pol = eig_cold_start(ub, ubf, 0);
  if (b >= n) eig_whole_space(pol);          // as eigen.hip: a block that spans the whole space is not filtered
  HostPool pool(3);
  RitzStep rr;
  std::vector<double> G((size_t)b * b), H((size_t)b * b), res(b, 1e300);
  int verdict = EIG_CONTINUE, round = 0;
  for (; round < max_rounds; ++round) {
    // the filter on the columns behind the locked ones, chunk by chunk, each chunk through its whole degree (as eigen.hip)
    const int nl = pol.nlock, ba = b - nl, deg_used = pol.deg, nch = eig_chunk_count(ba);
    const double e = (pol.ubf - pol.a) / 2.0, c = (pol.ubf + pol.a) / 2.0;
    printf("C %d %d %d", round, nl, nch);
    for (int q = 0; q < nch; ++q) {
      const int c0 = eig_chunk_start(ba, q), cw = eig_chunk_start(ba, q + 1) - c0;
      printf(" %d %d", c0, cw);
      if (c0 < 0 || cw <= 0 || cw > kEigChunkMax || c0 + cw > ba) { printf("\n"); return 1; }
      std::vector<float> X((size_t)n * cw), Y((size_t)n * cw), Z((size_t)n * cw);
      for (int i = 0; i < n; ++i) for (int j = 0; j < cw; ++j) X[(size_t)i * cw + j] = V[(size_t)i * b + nl + c0 + j];
      double sig = e / (pol.a0 - c);
      const double tau = 2.0 / sig;
      if (deg_used == 0) Y = X;
      else apply(pool, n, cw, A, X.data(), Y.data(), (float)(-c * sig / e), (float)(sig / e), nullptr, 0.f);
      for (int i = 2; i <= deg_used; ++i) {
        const double sn = 1.0 / (tau - sig);
        apply(pool, n, cw, A, Y.data(), Z.data(), (float)(-c * 2.0 * sn / e), (float)(2.0 * sn / e), X.data(), (float)(-sig * sn));
        X.swap(Y); Y.swap(Z);
        sig = sn;
      }
      apply(pool, n, cw, A, Y.data(), Z.data(), 0.f, 1.f, nullptr, 0.f);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < cw; ++j) { V[(size_t)i * b + nl + c0 + j] = Y[(size_t)i * cw + j]; LV[(size_t)i * b + nl + c0 + j] = Z[(size_t)i * cw + j]; }
    }
    printf("\n");
    pool.rows(b, 8, [&](int i) {
      for (int j = 0; j < b; ++j) {
        double g = 0.0, h = 0.0;
        for (int k = 0; k < n; ++k) { g += (double)V[(size_t)k * b + i] * V[(size_t)k * b + j]; h += (double)V[(size_t)k * b + i] * LV[(size_t)k * b + j]; }
        G[(size_t)i * b + j] = g; H[(size_t)i * b + j] = h;
      }
    });
    if (!rayleigh_ritz_host(b, G, H, pool, rr)) { printf("E -1 %d\n", round); return 0; }
    const double top = rr.th[rr.kept - 1];
    if (!pol.whole && eig_bound_short(pol, top)) { printf("E -2 %d\n", round); return 0; }      // the bound given is Gershgorin: never short
    // rotation V <- V W, L V <- L V W (accumulated in double, kept in float); residuals of the rotated block
    pool.rows(n, 16, [&](int i) {
      for (int j = 0; j < b; ++j) {
        double s = 0.0, t = 0.0;
        for (int k = 0; k < b; ++k) { s += (double)V[(size_t)i * b + k] * rr.wt[(size_t)j * b + k]; t += (double)LV[(size_t)i * b + k] * rr.wt[(size_t)j * b + k]; }
        Vn[(size_t)i * b + j] = (float)s; LVn[(size_t)i * b + j] = (float)t;
      }
    });
    for (int j = 0; j < b; ++j) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) { const float d = LVn[(size_t)i * b + j] - rr.thf[j] * Vn[(size_t)i * b + j]; s += (double)d * d; }
      res[j] = sqrt(s);
    }
    for (int i = 0; i < n; ++i) for (int j = rr.kept; j < b; ++j) Vn[(size_t)i * b + j] = uni();
    V.swap(Vn); LV.swap(LVn);
    const EigStep st = eig_round_step(pol, rr.th.data(), res.data(), m, b, rr.kept, tol, n, deg_used, tiles != 0, 0, nullptr);
    verdict = st.verdict;
    printf("R %d %d %d %d %d %d %.9g\n", round, deg_used, rr.kept, (int)st.verdict, st.nconv, st.lead, st.rmx);
    if (verdict != EIG_CONTINUE) { ++round; break; }
  }
  printf("E %d %d\n", verdict, round);
  for (int j = 0; j < b; ++j) printf("%.9g ", j < rr.kept ? (float)rr.th[j] : 0.f);
  printf("\n");
  for (auto x : V) printf("%.9g ", x);
  printf("\n");
  return 0;
}

int main(void) {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 's') { if (solve()) return 1; }
    else if (cmd == 'c') {        // c ba: the chunks of ba active columns
      int ba;
      if (!rdi(&ba)) return 1;
      const int nch = eig_chunk_count(ba);
      printf("K %d", nch);
      for (int q = 0; q <= nch; ++q) printf(" %d", eig_chunk_start(ba, q));
      printf("\n");
    } else return 1;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("eig_wide")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O3", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I",
                           os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(exe)])

    def run(text):
        out = subprocess.check_output([str(exe)], input=text + "\n", text=True)
        return [ln.split() for ln in out.strip().splitlines()]
    return run


@pytest.mark.parametrize("n", [256, 384, 512])
def test_host_symeig_wide_matches_lapack(n, monkeypatch):
    """mgp_host_symeig at the sizes a block of more than 256 columns hands it, with the checks test_host_symeig_matches_lapack
    makes at n <= 200: values, orthonormality and reconstruction against numpy on the same six kinds of matrix, the same bits on a
    second call -- and the same bits with 1, 3 and 16 host threads (the pool follows OMP_NUM_THREADS where it is set)."""
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(n)
    mats = [rng.standard_normal((n, n))]
    Bm = rng.standard_normal((n, n // 3))
    mats.append(Bm @ Bm.T)                                      # rank-deficient PSD
    mats.append(np.diag(np.repeat([1.0, 1.0 + 1e-12, 5.0], -(-n // 3))[:n]))   # (nearly) degenerate diagonal
    mats.append(np.zeros((n, n)))                               # every Householder step is the identity
    mats.append(np.diag(np.arange(1.0, n + 1)) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1))   # tridiagonal already
    mats.append(1e150 * rng.standard_normal((n, n)))            # the scaled norms / the guarded sqrt(a^2 + b^2)

    def solve(A):
        ev, V = np.empty(n), np.empty((n, n))
        assert lib.mgp_host_symeig(n, A.ctypes.data, ev.ctypes.data, V.ctypes.data) == 0
        return ev, V
    for Mx in mats:
        A = np.ascontiguousarray(0.5 * (Mx + Mx.T))
        monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
        ev, V = solve(A)
        ref = np.linalg.eigvalsh(A)
        scale = max(np.abs(ref).max(), 1e-300)
        assert np.all(np.diff(ev) >= 0)
        np.testing.assert_allclose(ev, ref, rtol=0, atol=1e-12 * scale * n)
        np.testing.assert_allclose(V.T @ V, np.eye(n), rtol=0, atol=1e-12 * n)
        np.testing.assert_allclose(V @ np.diag(ev) @ V.T, A, rtol=0, atol=1e-12 * scale * n)
        np.testing.assert_allclose(A @ V - V * ev, 0.0, rtol=0, atol=1e-12 * scale * n)      # residual of every pair
        ev2, V2 = solve(A)
        assert np.array_equal(ev, ev2) and np.array_equal(V, V2)
        for threads in ("1", "3", "16"):
            monkeypatch.setenv("OMP_NUM_THREADS", threads)
            ev3, V3 = solve(A)
            assert np.array_equal(ev, ev3) and np.array_equal(V, V3), threads


def test_chunk_rule_contracts(probe):
    """eig_chunk_start for every number of active columns up to the widest block: ceil(ba / 256) chunks that tile [0, ba) in order;
    every chunk starts on a multiple of 4 and every width but the last chunk's is a multiple of 4 (the last carries ba mod 4); no
    chunk above 256 columns; with more than one chunk they are balanced (widths within 7 of each other), so none is under the 48
    columns of the matrix-core SpMM; one chunk up to 256 columns is the whole block.  320 -> 160 + 160 and 300 -> 152 + 148."""
    rows = probe("\n".join("c %d" % ba for ba in range(1, 513)))
    assert len(rows) == 512
    for ba, r in zip(range(1, 513), rows):
        nch, starts = int(r[1]), [int(v) for v in r[2:]]
        widths = np.diff(starts)
        assert nch == -(-ba // 256) and len(starts) == nch + 1 and starts[0] == 0 and starts[-1] == ba, (ba, r)
        assert all(s % 4 == 0 for s in starts[:-1]) and all(w % 4 == 0 for w in widths[:-1]) and widths[-1] % 4 == ba % 4, (ba, r)
        assert widths.min() > 0 and widths.max() <= 256, (ba, r)
        if nch > 1:
            assert widths.max() - widths.min() <= 7 and widths.min() >= 48, (ba, r)
    by = {ba: [int(v) for v in r[2:]] for ba, r in zip(range(1, 513), rows)}
    assert by[320] == [0, 160, 320] and by[300] == [0, 152, 300] and by[256] == [0, 256] and by[512] == [0, 256, 512]


@pytest.fixture(scope="module")
def ring640():
    """Laplacian of the 640-node ring (eigenvalues 2 - 2 cos(2 pi k / 640): a clear low end, the 300 smallest reach 1.8 of 4)
    plus a seeded symmetric perturbation of 1e-3 per entry that splits its eigenvalue pairs, rounded to float32 (the matrix the
    probe sees); its float64 spectrum and Gershgorin bound."""
    rng = np.random.default_rng(11)
    A = 2.0 * np.eye(N)
    for i in range(N):
        A[i, (i + 1) % N] -= 1.0
        A[(i + 1) % N, i] -= 1.0
    P = rng.standard_normal((N, N)) * 1e-3
    A = (A + 0.5 * (P + P.T)).astype(np.float32)
    A64 = A.astype(np.float64)
    A64 = 0.5 * (A64 + A64.T)
    return dict(A=A, A64=A64, evals=np.linalg.eigvalsh(A64), ub=float(np.abs(A64).sum(1).max()) * (1.0 + 1e-6))


def test_wide_block_iteration_converges_and_keeps_the_chunk_contracts(probe, ring640):
    """m = 300 of 640, b = 384 (the library's own rule: the next multiple of 64 above 300 + 37), tol = 1e-5, filter bound =
    Gershgorin, the policy told that the matrix-core tiles are there (minimum 48 active columns per chunk).  The solve must end
    converged within the round budget with every one of the 300 pairs certified in float64 (an eigenvalue of the matrix within
    the pair's float64 residual of its Ritz value; that residual at most tol ub + F, F = 4 eps32 ||A||_2 ||v|| the rounding of
    the float mat-vec), the Ritz values ascending and within tol ub of numpy's; and at every round the filter ran on chunks that
    tile the active columns: locked run a multiple of 4, widths multiples of 4, none under 48, none above 256.
    Measured on the CPU: converged after 4 rounds (degrees 10, 8, 8, 8; leading converged runs 0, 208, 277, 300): rounds 0 and 1
    filter all 384 columns as 192 + 192, round 2 locks 208 and filters 176 in one chunk, round 3 locks 276 and filters 108;
    largest eigenvalue error 1.1e-7 against tol ub = 4.4e-5; worst float64 residual 0.76 of its bound."""
    tol = 1e-5
    text = "s %d %d %d %.9g %.17g %.17g 1 40 " % (N, B, M, tol, ring640["ub"], ring640["ub"]) + \
        " ".join("%.9g" % v for v in ring640["A"].ravel())
    rows = probe(text)
    chunks = [r for r in rows if r[0] == "C"]
    rounds = [r for r in rows if r[0] == "R"]
    end = next(i for i, r in enumerate(rows) if r[0] == "E")
    verdict, nrounds = int(rows[end][1]), int(rows[end][2])
    for r in rounds:
        print("round %s: degree %s kept %s verdict %s nconv %s lead %s rmax %s" % tuple(r[1:]))
    assert verdict == CONVERGED and nrounds <= 40 and len(chunks) == len(rounds) == nrounds, (verdict, nrounds)
    multi = 0
    for r in chunks:
        nl, nch = int(r[2]), int(r[3])
        c0 = [int(v) for v in r[4::2]]
        cw = [int(v) for v in r[5::2]]
        print("round %s: locked %d, chunks %s" % (r[1], nl, cw))
        assert nl % 4 == 0 and 0 <= nl <= M and len(cw) == nch == -(-(B - nl) // 256), r
        assert sum(cw) == B - nl and c0 == [int(v) for v in np.concatenate([[0], np.cumsum(cw)[:-1]])], r
        assert all(w % 4 == 0 and 48 <= w <= 256 for w in cw) and all(s % 4 == 0 for s in c0), r
        multi += nch > 1
    assert multi >= 1                                              # the wide path ran
    evals = np.array([float(v) for v in rows[end + 1]])
    block = np.array([float(v) for v in rows[end + 2]]).reshape(N, B)
    A64, w = ring640["A64"], ring640["evals"]
    assert np.all(np.diff(evals[:M]) >= 0)
    worst_val = np.abs(evals[:M] - w[:M]).max()
    print("largest eigenvalue error %.3e against tol ub %.3e" % (worst_val, tol * ring640["ub"]))
    assert worst_val <= tol * ring640["ub"]
    nrm2 = np.linalg.norm(A64, 2)
    worst = 0.0
    for j in range(M):
        v, th = block[:, j], evals[j]
        nv = np.linalg.norm(v)
        r = np.linalg.norm(A64 @ v - th * v)
        assert np.abs(w - th).min() <= r / nv, (j, th, r)
        F = 4 * EPS32 * nrm2 * nv
        assert r <= tol * ring640["ub"] + F, (j, r, tol * ring640["ub"], F)
        worst = max(worst, r / (tol * ring640["ub"] + F))
    print("rounds %d, worst float64 residual / bound %.3f" % (nrounds, worst))
    G = block[:, :M].T @ block[:, :M]
    assert np.abs(G - np.eye(M)).max() < 5e-5                     # the eigensolver tests' own orthonormality bar


def test_block_as_wide_as_the_whole_space_runs_unfiltered_rounds(probe):
    """n = 300, m = 250, b = n (the library's rule gives 320 columns, clamped to n): chunks 152 + 148.  Rayleigh-Ritz on the whole
    space is exact, so the policy runs rounds of degree 0 (eig_whole_space) on all columns, nothing locked, and converges within
    two: the first round on the random block, a second one on its orthonormalised rotation if the first rotation's rounding left
    residuals above tol (the probe accumulates its rotation in double and needs one).  Same matrix family, tolerance and float64 certificate as the 640 x 640 case.  With the filter left on
    (the state before eig_whole_space) this solve ran its whole round budget without one converged pair.
    Measured on the CPU: 1 round, worst float64 residual 0.64 of its bound."""
    n, m, b, tol = 300, 250, 300, 1e-5
    rng = np.random.default_rng(12)
    A = 2.0 * np.eye(n)
    for i in range(n):
        A[i, (i + 1) % n] -= 1.0
        A[(i + 1) % n, i] -= 1.0
    P = rng.standard_normal((n, n)) * 1e-3
    A = (A + 0.5 * (P + P.T)).astype(np.float32)
    A64 = A.astype(np.float64)
    A64 = 0.5 * (A64 + A64.T)
    w = np.linalg.eigvalsh(A64)
    ub = float(np.abs(A64).sum(1).max()) * (1.0 + 1e-6)
    rows = probe("s %d %d %d %.9g %.17g %.17g 1 40 " % (n, b, m, tol, ub, ub) + " ".join("%.9g" % v for v in A.ravel()))
    chunks = [r for r in rows if r[0] == "C"]
    rounds = [r for r in rows if r[0] == "R"]
    end = next(i for i, r in enumerate(rows) if r[0] == "E")
    for r in rounds:
        print("round %s: degree %s kept %s verdict %s nconv %s lead %s rmax %s" % tuple(r[1:]))
    assert int(rows[end][1]) == CONVERGED and int(rows[end][2]) <= 2, rows[end]
    assert all(int(r[2]) == 0 for r in rounds)                                  # degree 0 in every round
    assert all([int(v) for v in r[2:]] == [0, 2, 0, 152, 152, 148] for r in chunks), chunks
    evals = np.array([float(v) for v in rows[end + 1]])
    block = np.array([float(v) for v in rows[end + 2]]).reshape(n, b)
    assert np.all(np.diff(evals[:m]) >= 0) and np.abs(evals[:m] - w[:m]).max() <= tol * ub
    nrm2 = np.linalg.norm(A64, 2)
    worst = 0.0
    for j in range(m):
        v, th = block[:, j], evals[j]
        r = np.linalg.norm(A64 @ v - th * v)
        bound = tol * ub + 4 * EPS32 * nrm2 * np.linalg.norm(v)
        assert r <= bound, (j, r, bound)
        worst = max(worst, r / bound)
    print("worst float64 residual / bound %.3f" % worst)
    assert np.abs(block[:, :m].T @ block[:, :m] - np.eye(m)).max() < 5e-5
