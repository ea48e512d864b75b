"""The eigensolver's round policy (manifold_gp_amd/csrc/eig_policy.h) and host algebra (eig_host.h) on the CPU: both headers
compile with a host compiler alone, so a small C++ probe runs the whole Chebyshev-filtered block iteration on a dense 96 x 96
matrix -- float vectors, a float dense mat-vec, double Gram blocks -- and takes EVERY decision (start, warm start, short bound,
the step after a round) and every Rayleigh-Ritz step from the two headers: the functions the driver in eigen.hip calls.

The oracle is numpy.linalg.eigvalsh in float64 on the matrix the probe sees and the residual theorem for symmetric matrices
(an eigenvalue lies within ||A v - theta v|| / ||v|| of theta), never a transliteration of the policy.  The contracts of the step
function are the ones stated in docs/kernels/eigen.md."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
EPS32 = float(np.finfo(np.float32).eps)
N, B, M = 96, 16, 6
CONVERGED, FLOOR, CONTINUE = 1, 2, 0

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

// Y[:, j] = ca X[:, j] + cb (A X)[:, j] (+ cc Z[:, j]) in float, on `w` columns
static void apply(int n, int w, const std::vector<float>& A, const float* X, float* Y, float ca, float cb, const float* Z, float cc) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < w; ++j) {
      float t = 0.f;
      for (int k = 0; k < n; ++k) t += A[(size_t)i * n + k] * X[(size_t)k * w + j];
      Y[(size_t)i * w + j] = ca * X[(size_t)i * w + j] + cb * t + (Z ? cc * Z[(size_t)i * w + j] : 0.f);
    }
}

static void print_state(const EigPolicy& s) { printf("%d %.17g %.17g %.17g %d %d", s.kCap, s.ubf, s.a, s.a0, s.deg, s.nlock); }

// solve: n b m tol ub ubf user_degree max_rounds warm, A [n x n], (warm: evals [b], block [n x b])
static int solve() {
  int n, b, m, user_degree, max_rounds, warm; double tol, ub, ubf, v;
  if (!rdi(&n) || !rdi(&b) || !rdi(&m) || !rd(&tol) || !rd(&ub) || !rd(&ubf) || !rdi(&user_degree) || !rdi(&max_rounds) || !rdi(&warm)) return 1;
  std::vector<float> A((size_t)n * n), V((size_t)n * b), LV((size_t)n * b), Vn((size_t)n * b), LVn((size_t)n * b), wev(b);
  for (auto& x : A) { if (!rd(&v)) return 1; x = (float)v; }
  g_rng = 1337;
  for (auto& x : V) x = uni();
  EigPolicy pol = eig_cold_start(ub, ubf, user_degree);
  if (warm) {
    for (auto& x : wev) { if (!rd(&v)) return 1; x = (float)v; }
    for (auto& x : V) { if (!rd(&v)) return 1; x = (float)v; }
    eig_warm_start(pol, wev.data(), b, m, user_degree);
  }
  printf("S "); print_state(pol); printf("\n");
  HostPool pool(1);
  RitzStep rr;
  std::vector<double> G((size_t)b * b), H((size_t)b * b), res(b, 1e300);
  int verdict = EIG_CONTINUE, round = 0;
  for (; round < max_rounds; ++round) {
    // scaled Chebyshev filter of degree pol.deg damping [a, ubf], normalised at a0, on the columns behind the locked ones
    const int nl = pol.nlock, ba = b - nl, deg_used = pol.deg;
    std::vector<float> X((size_t)n * ba), Y((size_t)n * ba), Z((size_t)n * ba);
    for (int i = 0; i < n; ++i) for (int j = 0; j < ba; ++j) X[(size_t)i * ba + j] = V[(size_t)i * b + nl + j];
    const double e = (pol.ubf - pol.a) / 2.0, c = (pol.ubf + pol.a) / 2.0;
    double sig = e / (pol.a0 - c);
    const double tau = 2.0 / sig;
    apply(n, ba, A, X.data(), Y.data(), (float)(-c * sig / e), (float)(sig / e), nullptr, 0.f);
    for (int i = 2; i <= deg_used; ++i) {
      const double sn = 1.0 / (tau - sig);
      apply(n, ba, A, Y.data(), Z.data(), (float)(-c * 2.0 * sn / e), (float)(2.0 * sn / e), X.data(), (float)(-sig * sn));
      X.swap(Y); Y.swap(Z);
      sig = sn;
    }
    for (int i = 0; i < n; ++i) for (int j = 0; j < ba; ++j) V[(size_t)i * b + nl + j] = Y[(size_t)i * ba + j];
    apply(n, b, A, V.data(), LV.data(), 0.f, 1.f, nullptr, 0.f);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j) {
        double g = 0.0, h = 0.0;
        for (int k = 0; k < n; ++k) { g += (double)V[(size_t)k * b + i] * V[(size_t)k * b + j]; h += (double)V[(size_t)k * b + i] * LV[(size_t)k * b + j]; }
        G[(size_t)i * b + j] = g; H[(size_t)i * b + j] = h;
      }
    if (!rayleigh_ritz_host(b, G, H, pool, rr)) { printf("E -1 %d\n", round); return 0; }
    const double top = rr.th[rr.kept - 1], ubf_before = pol.ubf;
    if (eig_bound_short(pol, top)) {
      pol = eig_cold_start(pol.ub, pol.ub, user_degree);
      for (auto& x : V) x = uni();
      printf("R %d 1 %d %d %.17g %.17g 0 0 ", round, deg_used, rr.kept, top, ubf_before); print_state(pol); printf("\n");
      continue;
    }
    // rotation V <- V W, L V <- L V W (accumulated in double, kept in float); residuals of the rotated block
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < b; ++j) {
        double s = 0.0, t = 0.0;
        for (int k = 0; k < b; ++k) { s += (double)V[(size_t)i * b + k] * rr.wt[(size_t)j * b + k]; t += (double)LV[(size_t)i * b + k] * rr.wt[(size_t)j * b + k]; }
        Vn[(size_t)i * b + j] = (float)s; LVn[(size_t)i * b + j] = (float)t;
      }
    for (int j = 0; j < b; ++j) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) { const float d = LVn[(size_t)i * b + j] - rr.thf[j] * Vn[(size_t)i * b + j]; s += (double)d * d; }
      res[j] = sqrt(s);
    }
    for (int i = 0; i < n; ++i) for (int j = rr.kept; j < b; ++j) Vn[(size_t)i * b + j] = uni();
    V.swap(Vn); LV.swap(LVn);
    const EigStep st = eig_round_step(pol, rr.th.data(), res.data(), m, b, rr.kept, tol, n, deg_used, false, user_degree, nullptr);
    verdict = st.verdict;
    printf("R %d 0 %d %d %.17g %.17g %d %d ", round, deg_used, rr.kept, top, ubf_before, (int)st.verdict, st.nconv); print_state(pol); printf("\n");
    if (verdict != EIG_CONTINUE) { ++round; break; }
  }
  printf("E %d %d\n", verdict, round);
  for (int j = 0; j < b; ++j) printf("%.9g ", j < rr.kept ? (float)rr.th[j] : 0.f);
  printf("\n");
  for (auto x : V) printf("%.9g ", x);
  printf("\n");
  return 0;
}

// step: ub ubf user_degree top_prev rmax_prev nconv_prev | m b kept tol n deg_used tiles | th [kept] | res [b]
static int step() {
  double ub, ubf, top_prev, rmax_prev, tol, nn; int user_degree, nconv_prev, m, b, kept, deg_used, tiles;
  if (!rd(&ub) || !rd(&ubf) || !rdi(&user_degree) || !rd(&top_prev) || !rd(&rmax_prev) || !rdi(&nconv_prev) || !rdi(&m) || !rdi(&b) ||
      !rdi(&kept) || !rd(&tol) || !rd(&nn) || !rdi(&deg_used) || !rdi(&tiles)) return 1;
  std::vector<double> th(kept), res(b);
  for (auto& x : th) if (!rd(&x)) return 1;
  for (auto& x : res) if (!rd(&x)) return 1;
  EigPolicy pol = eig_cold_start(ub, ubf, user_degree);
  pol.top_prev = top_prev; pol.rmax_prev = rmax_prev; pol.nconv_prev = nconv_prev;
  const EigStep st = eig_round_step(pol, th.data(), res.data(), m, b, kept, tol, (int64_t)nn, deg_used, tiles != 0, user_degree, nullptr);
  printf("P %d %d %d %.17g ", (int)st.verdict, st.nconv, st.lead, st.rmx); print_state(pol); printf("\n");
  return 0;
}

int main(void) {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 's') { if (solve()) return 1; }
    else if (cmd == 'p') { if (step()) return 1; }
    else if (cmd == 'i') {
      double ub, ubf; int ud;
      if (!rd(&ub) || !rd(&ubf) || !rdi(&ud)) return 1;
      printf("I "); print_state(eig_cold_start(ub, ubf, ud)); printf("\n");
    } else return 1;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("eig_policy")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-I",
                           os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(exe)])

    def run(text):
        out = subprocess.check_output([str(exe)], input=text + "\n", text=True)
        return [ln.split() for ln in out.strip().splitlines()]
    return run


STATE = ("kCap", "ubf", "a", "a0", "deg", "nlock")


def _state(tok):
    return dict(kCap=int(tok[0]), ubf=float(tok[1]), a=float(tok[2]), a0=float(tok[3]), deg=int(tok[4]), nlock=int(tok[5]))


@pytest.fixture(scope="module")
def ring():
    """Symmetric normalised Laplacian of a 96-node ring with seeded random positive weights, rounded to float32 (the matrix the
    probe sees); its float64 spectrum and Gershgorin bound."""
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, N)
    W = np.zeros((N, N))
    for i in range(N):
        W[i, (i + 1) % N] = W[(i + 1) % N, i] = w[i]
    d = W.sum(1)
    A = (np.eye(N) - W / np.sqrt(np.outer(d, d))).astype(np.float32)
    A64 = A.astype(np.float64)
    A64 = 0.5 * (A64 + A64.T)
    return dict(A=A, A64=A64, evals=np.linalg.eigvalsh(A64), ub=float(np.abs(A64).sum(1).max()) * (1.0 + 1e-6))


def _solve_text(ring, tol, ubf, max_rounds=40, warm=None, user_degree=0):
    head = "s %d %d %d %.9g %.17g %.17g %d %d %d " % (N, B, M, tol, ring["ub"], ubf, user_degree, max_rounds, 0 if warm is None else 1)
    body = " ".join("%.9g" % v for v in ring["A"].ravel())
    if warm is not None:
        body += " " + " ".join("%.9g" % v for v in np.concatenate([warm["evals"], warm["block"].ravel()]))
    return head + body


def _parse_solve(rows):
    out = dict(start=_state(rows[0][1:]), rounds=[])
    assert rows[0][0] == "S"
    i = 1
    while rows[i][0] == "R":
        t = rows[i]
        out["rounds"].append(dict(round=int(t[1]), short=int(t[2]), deg_used=int(t[3]), kept=int(t[4]), top=float(t[5]),
                                  ubf_before=float(t[6]), verdict=int(t[7]), nconv=int(t[8]), state=_state(t[9:])))
        i += 1
    assert rows[i][0] == "E"
    out["verdict"], out["nrounds"] = int(rows[i][1]), int(rows[i][2])
    out["evals"] = np.array([float(v) for v in rows[i + 1]])
    out["block"] = np.array([float(v) for v in rows[i + 2]]).reshape(N, B)
    return out, rows[i + 3:]


def _check_converged(ring, sol, tol):
    """Ended converged within the round budget; every returned pair certified in float64: by the residual theorem an eigenvalue
    of the matrix lies within the pair's float64 residual of its Ritz value, and that residual is at most tol ub + F with
    F = 4 eps32 ||A||_2 ||v|| the fp32 rounding of the probe's mat-vec (the form of the CG floor in test_gpu_solver_contract.py)."""
    assert sol["verdict"] == CONVERGED and sol["nrounds"] <= 40, (sol["verdict"], sol["nrounds"])
    A64, w = ring["A64"], ring["evals"]
    worst = 0.0
    for j in range(M):
        v, th = sol["block"][:, j], sol["evals"][j]
        r = np.linalg.norm(A64 @ v - th * v) / np.linalg.norm(v)
        assert np.abs(w - th).min() <= r, (j, th, r)
        F = 4 * EPS32 * np.linalg.norm(A64, 2) * np.linalg.norm(v)
        print("pair %d: theta %.9g float64 residual %.3e bound %.3e" % (j, th, r * np.linalg.norm(v), tol * ring["ub"] + F))
        assert r * np.linalg.norm(v) <= tol * ring["ub"] + F, (j, r, tol * ring["ub"], F)
        worst = max(worst, r * np.linalg.norm(v) / (tol * ring["ub"] + F))
    return worst


@pytest.fixture(scope="module")
def cold(probe, ring):
    sol, rest = _parse_solve(probe(_solve_text(ring, 1e-4, ring["ub"])))
    assert not rest
    return sol


def test_cold_solve_converges_to_certified_pairs(ring, cold):
    """tol = 1e-4, filter bound = Gershgorin.  Measured on the CPU: converged after 3 rounds; the largest float64 residual of the
    six returned pairs is 1.67e-5 against the bound tol ub + F = 2.185e-4 (0.077 of it; F = 9.5e-7)."""
    assert cold["start"] == dict(kCap=200, ubf=ring["ub"], a=ring["ub"] / 4, a0=0.0, deg=10, nlock=0)
    assert not any(r["short"] for r in cold["rounds"])
    worst = _check_converged(ring, cold, 1e-4)
    print("rounds %d, worst residual / bound %.3f" % (cold["nrounds"], worst))


def test_short_bound_is_proven_and_answered_with_gershgorin(probe, ring):
    """Filter bound = half of lambda_max: a round must report it short -- with a Ritz value ABOVE the bound, the proof the policy
    relies on --, the state must come back as the cold state on the Gershgorin bound with the cap at 200, and the solve then
    converges to certified pairs like the cold one."""
    ubf = 0.5 * float(ring["evals"][-1])
    sol, rest = _parse_solve(probe(_solve_text(ring, 1e-4, ubf)))
    assert not rest
    assert sol["start"]["ubf"] == ubf and 100 <= sol["start"]["kCap"] <= 200
    short = [r for r in sol["rounds"] if r["short"]]
    assert len(short) == 1, [r["round"] for r in short]
    assert short[0]["ubf_before"] == ubf and short[0]["top"] > ubf, short[0]
    assert short[0]["top"] <= ring["evals"][-1] * (1 + 1e-6)              # ... and a Ritz value it is
    assert short[0]["state"] == dict(kCap=200, ubf=ring["ub"], a=ring["ub"] / 4, a0=0.0, deg=10, nlock=0), short[0]["state"]
    assert all(r["state"]["ubf"] == ring["ub"] and r["state"]["kCap"] == 200 for r in sol["rounds"][short[0]["round"]:])
    _check_converged(ring, sol, 1e-4)


def test_warm_start_takes_its_filter_from_the_warm_ritz_values(probe, ring, cold):
    """The converged block and Ritz values of the cold solve as the warm start on the same matrix: no more rounds than the cold
    run, and the first round is a full-strength one: damping interval from just above the block's largest Ritz value, degree from
    the gap, inside [8, kCap]."""
    warm = dict(evals=cold["evals"], block=cold["block"])
    sol, rest = _parse_solve(probe(_solve_text(ring, 1e-4, ring["ub"], warm=warm)))
    assert not rest
    st = sol["start"]
    assert cold["evals"][B - 1] < st["a"] < ring["ub"] and st["a"] != ring["ub"] / 4, st
    assert st["a0"] <= 0.0 and 8 <= st["deg"] <= st["kCap"] == 200, st
    assert sol["rounds"][0]["deg_used"] == st["deg"]
    assert sol["nrounds"] <= cold["nrounds"], (sol["nrounds"], cold["nrounds"])
    _check_converged(ring, sol, 1e-4)
    # a user degree is kept
    sol, _ = _parse_solve(probe(_solve_text(ring, 1e-4, ring["ub"], warm=warm, user_degree=23, max_rounds=2)))
    assert sol["start"]["deg"] == 23 and all(r["deg_used"] == 23 for r in sol["rounds"])


def _step_text(ub, ubf, th, res, m, b, tol, user_degree=0, top_prev=1e300, rmax_prev=1e300, nconv_prev=0, n=60000, deg_used=10,
               tiles=0):
    return "p %.17g %.17g %d %.17g %.17g %d %d %d %d %.17g %d %d %d " % (ub, ubf, user_degree, top_prev, rmax_prev, nconv_prev, m, b,
                                                                         len(th), tol, n, deg_used, tiles) + \
        " ".join("%.17g" % v for v in list(th) + list(res))


def _steps(probe, texts):
    rows = probe("\n".join(texts))
    assert len(rows) == len(texts) and all(r[0] == "P" for r in rows)
    return [dict(verdict=int(r[1]), nconv=int(r[2]), lead=int(r[3]), rmx=float(r[4]), **_state(r[5:])) for r in rows]


def test_step_contracts_degree_cap_and_locking(probe):
    """docs/kernels/eigen.md: the adaptive degree lies in [8, kCap] with kCap in [100, 200]; a user degree is returned unchanged;
    the locked run is a multiple of 4 columns, leaves at least 8 columns in the filter and, where the CSR carries the matrix-core
    tile image and b >= 48, at least 48."""
    ub, tol = 2.0, 1e-5
    rows = probe("\n".join("i %.17g %.17g 0" % (ub, ub * f) for f in np.linspace(0.01, 1.0, 34)))
    caps = [_state(r[1:])["kCap"] for r in rows]
    assert all(100 <= c <= 200 for c in caps) and caps[-1] == 200 and min(caps) == 100, caps
    rng = np.random.default_rng(2)
    texts, cases = [], []
    for b, m in ((16, 6), (64, 24), (64, 50), (128, 100), (40, 30), (12, 9)):
        for tiles in (0, 1):
            for lead in sorted({0, 1, 3, 4, 5, m // 2, m - 3, m - 1}):
                for user_degree in (0, 37):
                    ubf = ub * rng.uniform(0.3, 1.0)
                    th = np.sort(rng.uniform(0, 0.2 * ubf, b)) * 10.0 ** rng.uniform(-6, 0)
                    res = tol * ub * 10.0 ** rng.uniform(0.1, 3, b)
                    res[:lead] = tol * ub * rng.uniform(0, 1, lead)
                    texts.append(_step_text(ub, ubf, th, res, m, b, tol, user_degree=user_degree, tiles=tiles,
                                            n=int(10 ** rng.uniform(2, 7))))
                    cases.append((b, m, tiles, lead, user_degree))
    for (b, m, tiles, lead, user_degree), r in zip(cases, _steps(probe, texts)):
        assert r["verdict"] == CONTINUE and r["lead"] == lead and r["nconv"] >= lead, (b, m, lead, r)
        assert 100 <= r["kCap"] <= 200
        assert r["deg"] == 37 if user_degree else 8 <= r["deg"] <= r["kCap"], r
        assert r["nlock"] % 4 == 0 and 0 <= r["nlock"] <= lead and b - r["nlock"] >= 8, (b, lead, r)
        if tiles and b >= 48:
            assert b - r["nlock"] >= 48, (b, lead, r)


def test_step_contracts_exits(probe):
    """The observed floor exit (a cap-degree round that neither halves the largest wanted residual nor gains a pair) applies only
    within floor_guard = max(50 tol, 2e-5) of ub; m pairs under tol ub is convergence; a block of rank below m neither converges nor
    is at the floor; a user degree disables the predicted exit."""
    ub, tol, b, m = 2.0, 1e-6, 16, 6
    guard = max(50 * tol, 2e-5) * ub
    th = np.linspace(0.0, 0.5, b)

    def res_with(rmx, nconv=2):
        r = np.full(b, 10 * guard)
        r[:m] = rmx
        r[:nconv] = 0.5 * tol * ub
        return r
    cap = dict(deg_used=200, rmax_prev=1.2 * guard, nconv_prev=2)
    texts = [
        _step_text(ub, ub, th, res_with(0.999 * guard), m, b, tol, **cap),                 # 0 at the floor, inside the guard
        _step_text(ub, ub, th, res_with(1.001 * guard), m, b, tol, **cap),                 # 1 the same round just outside it
        _step_text(ub, ub, th, res_with(0.5 * guard), m, b, tol, **cap),                   # 2 halved (0.5 / 1.2): no floor
        _step_text(ub, ub, th, res_with(0.999 * guard, nconv=3), m, b, tol, **cap),        # 3 gained a pair: no floor
        _step_text(ub, ub, th, res_with(0.999 * guard), m, b, tol, deg_used=199, rmax_prev=1.2 * guard, nconv_prev=2),   # 4 not a cap round
        _step_text(ub, ub, th, res_with(tol * ub, nconv=m), m, b, tol),                    # 5 exactly m pairs at / under tol ub
        _step_text(ub, ub, th[:m - 1], res_with(0.0, nconv=m), m, b, tol, **cap),          # 6 rank m - 1, residuals all zero
        _step_text(ub, ub, th[:m - 1], res_with(0.999 * guard), m, b, tol, **cap),         # 7 rank m - 1 at the "floor"
    ]
    # predicted exit: the wanted block in a cluster with its guards (gap 1e-9 of the interval), halved residual: not observed
    thc = np.concatenate([np.zeros(m), np.full(b - m, 1e-9)])
    texts.append(_step_text(ub, ub, thc, res_with(0.5 * guard), m, b, tol, **cap))         # 8 predicted floor
    texts.append(_step_text(ub, ub, thc, res_with(0.5 * guard), m, b, tol, user_degree=200, **cap))   # 9 user degree: runs on
    texts.append(_step_text(ub, ub, thc, res_with(1.001 * guard), m, b, tol, **cap))       # 10 outside the guard: runs on
    r = _steps(probe, texts)
    assert r[0]["verdict"] == FLOOR and r[0]["nconv"] == 2, r[0]
    for i in (1, 2, 3, 4):
        assert r[i]["verdict"] == CONTINUE, (i, r[i])
    assert r[5]["verdict"] == CONVERGED and r[5]["nconv"] == m, r[5]
    for i in (6, 7):
        assert r[i]["verdict"] == CONTINUE and r[i]["nconv"] == 0 and r[i]["nlock"] == 0, (i, r[i])
    assert r[8]["verdict"] == FLOOR, r[8]
    assert r[9]["verdict"] == CONTINUE and r[9]["deg"] == 200, r[9]
    assert r[10]["verdict"] == CONTINUE and r[10]["deg"] == 200, r[10]
