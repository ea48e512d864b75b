"""The folded CG step (docs/kernels/cg.md, round 6) on the CPU: the identity it rests on, the recurrence with either delta through
the host-compiled rule, and the gating of cg_choose.

With Q2 = scale P B^2 P (B = tau I + L_sym symmetric, ONE vector P as pre and post) and u = r,
    u . A u = c |B P u|^2            (form 0: A = c P B^2 P,     c = scale)
    u . A u = gamma + c |B P u|^2    (form 2: A = I + c P B^2 P, c = noise x scale, gamma = r . r)
so delta is known after the FIRST SpMV of the apply.  The references are float64 numpy; nothing here is read off the kernels."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
EPS32 = float(np.finfo(np.float32).eps)


# ----------------------------------------------------------------------------- the identity, float64, golden dumbbell
@pytest.fixture(scope="module")
def dumbbell_B():
    """(norm -> (B = tau I + L_sym dense float64, P or None)) on the golden dumbbell, nu = 2."""
    from oracle.laplacian import LaplacianOracle
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "dumbbell_k10_loop.npz")))
    n = g["train_x"].shape[0]
    tau = 2.0 * 2 / float(g["kappa"]) ** 2
    out = {"y": g["train_y"].astype(np.float64)}
    for norm in ("symmetric", "randomwalk"):
        lo = LaplacianOracle(g["edge_value"], g["edge_index"], n, float(g["eps"]), norm, bool(g["self_loops"]), dtype=np.float64)
        B = tau * np.eye(n) + lo.dense_symmetric()
        assert np.abs(B - B.T).max() == 0.0
        out[norm] = (B, np.sqrt(lo.degree) if norm == "randomwalk" else None)
    return out


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("norm", ["symmetric", "randomwalk"])
def test_delta_identity_float64(dumbbell_B, norm, form):
    B, P = dumbbell_B[norm]
    n = B.shape[0]
    scale, noise = 0.7, 1e-2
    c = noise * scale if form == 2 else scale
    rng = np.random.default_rng(3)
    for u in (dumbbell_B["y"], rng.standard_normal(n), np.eye(n)[:, 17]):
        Pu = u if P is None else P * u
        t = B @ Pu                                   # what the first SpMV writes
        Bt = B @ t
        Au = c * (Bt if P is None else P * Bt) + (u if form == 2 else 0.0)
        uAu = float(u @ Au)
        gamma = float(u @ u)
        folded = (gamma if form == 2 else 0.0) + c * float(t @ t)
        assert abs(uAu - folded) <= 1e-12 * abs(uAu), (norm, form, uAu, folded)


# ----------------------------------------------------------------------------- the recurrence with either delta (cg_rule.h)
RULE_PROBE = r"""
#include <stdio.h>
#include <vector>
#include "cg_rule.h"
typedef std::vector<float> V;
static int N;
static float dot(const V& a, const V& b) { float t = 0.f; for (int i = 0; i < N; ++i) t += a[i] * b[i]; return t; }
int main(void) {
  // a solve: N form folded tol max_iter c, B (row major), P, b -- A = [I +] c P B^2 P, delta = u . A u or [gamma +] c |B P u|^2
  int form, folded, max_iter; float tol, c;
  while (scanf("%d %d %d %f %d %f", &N, &form, &folded, &tol, &max_iter, &c) == 6) {
    std::vector<V> B(N, V(N));
    V P(N), b(N), x(N, 0.f), p(N, 0.f), s(N, 0.f), r(N), w(N), t(N), us(N);
    for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) if (scanf("%f", &B[i][j]) != 1) return 1;
    for (int i = 0; i < N; ++i) if (scanf("%f", &P[i]) != 1) return 1;
    for (int i = 0; i < N; ++i) if (scanf("%f", &b[i]) != 1) return 1;
    r = b;
    float gamma_old = 0.f, alpha_old = 0.f, bb = 0.f, rel = 0.f;
    CgStop st = {0, 0};
    int steps = 0;
    for (;; ++steps) {
      for (int i = 0; i < N; ++i) us[i] = P[i] * r[i];
      for (int i = 0; i < N; ++i) t[i] = dot(B[i], us);                                   // first SpMV: t = B P u
      for (int i = 0; i < N; ++i) w[i] = c * (P[i] * dot(B[i], t)) + (form == 2 ? r[i] : 0.f);   // second: w = A u
      const float gamma = dot(r, r);
      const float delta = folded ? (form == 2 ? gamma : 0.f) + c * dot(t, t) : dot(r, w);
      if (steps == 0) bb = gamma;
      rel = cg_rel(gamma, bb);
      st = cg_stop(1, 0, max_iter, tol, steps + 1, rel);
      const CgCoef k = cg_coef(steps == 0, cg_frozen(1, tol, rel), gamma, delta, gamma_old, alpha_old);
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
    printf("%d %d %.9g\n", steps, st.status, rel);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def rule_probe(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("cg_fold_rule")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(RULE_PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src),
                           "-o", str(exe)])

    def run(lines):
        out = subprocess.check_output([str(exe)], input="\n".join(lines) + "\n", text=True)
        return [[float(v) for v in ln.split()] for ln in out.strip().splitlines()]
    return run


def _system(n, tau, seed):
    """B = tau I + L_sym of a weighted ring with chords (float32, as the probe sees it), P in [0.8, 1.25], Gaussian b."""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    for i in range(n):
        for d in (1, 2, 5):
            w = rng.uniform(0.2, 1.0)
            W[i, (i + d) % n] += w
            W[(i + d) % n, i] += w
    deg = W.sum(1)
    L = np.eye(n) - W / np.sqrt(np.outer(deg, deg))
    B = (tau * np.eye(n) + L).astype(np.float32)
    B = 0.5 * (B + B.T)
    return B, rng.uniform(0.8, 1.25, n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


# tau sets the conditioning: cond(P B^2 P) <= 2.5 ((tau + 2) / tau)^2 = 6, 61, 510 -- from a solve of a few steps to one of tens.  The
# floor of a float32 solve is F <= 4 eps32 cond(A) = 1.2e-4 at the worst of them, so tol = 1e-3 keeps F <= tol / 4 (not vacuous)
@pytest.mark.parametrize("tau", [4.0, 0.5, 0.15])
@pytest.mark.parametrize("form", [0, 2])
def test_recurrence_with_either_delta(rule_probe, form, tau):
    n, tol = 48, 1e-3
    B, P, b = _system(n, tau, seed=int(10 * tau) + form)
    c = 0.7 if form == 0 else 0.7 * (1e-2 if tau > 1 else 30.0)      # form 2: far from the identity at the small tau
    line = lambda folded: "%d %d %d %.9g 500 %.9g " % (n, form, folded, tol, c) + \
        " ".join("%.9g" % v for v in np.concatenate([B.ravel(), P, b]))
    rows = rule_probe([line(0), line(1)])
    B64, P64, b64 = B.astype(np.float64), P.astype(np.float64), b.astype(np.float64)
    A = np.float64(np.float32(c)) * (P64[:, None] * (B64 @ B64) * P64[None, :]) + (np.eye(n) if form == 2 else 0.0)
    steps = []
    for row in rows:
        x, k, status = np.array(row[:n]), int(row[n]), int(row[n + 1])
        true_rel = np.linalg.norm(b64 - A @ x) / np.linalg.norm(b64)
        F = 4 * EPS32 * np.linalg.norm(A, 2) * np.linalg.norm(x) / np.linalg.norm(b64)
        print("form %d tau %g: steps %d true_rel %.3g F %.3g" % (form, tau, k, true_rel, F))
        assert status == 1
        assert F <= tol / 4 and true_rel <= 2 * tol + F, (true_rel, F)        # contract C1 (tests/test_gpu_solver_contract.py)
        steps.append(k)
    assert steps[0] == steps[1], steps
    x0, x1 = np.array(rows[0][:n]), np.array(rows[1][:n])
    assert np.abs(x0 - x1).max() <= 4 * tol * np.abs(x0).max()               # both within tol-level residual of one system


# ----------------------------------------------------------------------------- the gating of cg_choose
POLICY_PROBE = r"""
#include <stdio.h>
#include <sys/mman.h>
#include "cg_policy.h"
int main(void) {
  // n C nb_loc is_dist minv pre post form nu cc tile pre_is_post tile_rows | complex_shift init_free fold_update
  long long n; int C, nb, d, mi, pr, po, form, nu, tp, pip, tr, kcx, kif, kfo; double cc;
  while (scanf("%lld %d %d %d %d %d %d %d %d %lf %d %d %d %d %d %d", &n, &C, &nb, &d, &mi, &pr, &po, &form, &nu, &cc, &tp, &pip, &tr,
               &kcx, &kif, &kfo) == 16) {
    CgShape sh{};
    sh.n = n; sh.world = 1; sh.is_dist = d != 0; sh.C = C; sh.nb_loc = nb; sh.nb4 = (C == 1 && !d) ? 940 : 0;
    sh.has_minv = mi != 0; sh.has_pre = pr != 0; sh.has_post = po != 0; sh.form = form; sh.nu = nu; sh.noise_scale = (float)cc;
    sh.stop_mode = 1; sh.tile_plan = tp != 0; sh.pre_is_post = pip != 0; sh.tile_rows = tr;
    CgKnobs k;
    k.complex_shift = kcx; k.init_free = kif; k.fold_update = kfo;
    const CgChoice c = cg_choose(sh, k);
    const size_t counted = cg_workspace_bytes(sh, c);
    char* base = (char*)mmap(nullptr, counted, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) return 1;
    MgpArena ar(base, counted);
    CgBuffers b;
    cg_carve(ar, sh, c, &b);
    const void* p[] = {b.x, b.r, b.ubuf, b.w, b.p, b.s, b.usbuf, b.op_work, b.pd_gamma, b.pd_rr, b.pd_delta, b.blk, b.tot, b.xacc, b.rbuf,
                       b.tbuf, b.rpart, b.xacc64, b.t64, b.work64, b.rpart64, b.cz, b.cr, b.cp, b.cs, b.u4, b.w4, b.y4, b.op_work4, b.pd4,
                       b.pd_g, b.sc, b.pd_bb, b.arrive};
    printf("%d %d %d %d %d %lld %d %d %d %d %d %d %d %zu", c.fold ? 1 : 0, c.TC, c.TS, c.CQ, c.TSQ, (long long)c.rows_per_block, c.nbv, c.nbs,
           c.reduce_once ? 1 : 0, c.upd_quads, c.c1_family ? 1 : 0, c.cx ? 1 : 0, c.init_free ? 1 : 0, counted);
    for (const void* q : p) printf(" %lld", q ? (long long)((const char*)q - base) : -1LL);
    printf("\n");
    munmap(base, counted);
  }
  return 0;
}
"""

QUALIFYING = dict(n=60000, C=1, nb=235, dist=0, minv=0, pre=1, post=1, form=2, nu=2, cc=0.007, tile=1, pip=1, tr=64, kcx=1, kif=1, kfo=1)


def _line(**kw):
    v = dict(QUALIFYING, **kw)
    return "%d %d %d %d %d %d %d %d %d %.9g %d %d %d %d %d %d" % tuple(v[k] for k in (
        "n", "C", "nb", "dist", "minv", "pre", "post", "form", "nu", "cc", "tile", "pip", "tr", "kcx", "kif", "kfo"))


@pytest.fixture(scope="module")
def policy_probe(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("cg_fold_policy")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(POLICY_PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.check_output([str(exe)], input="\n".join(lines) + "\n", text=True)
        rows = [[int(v) for v in ln.split()] for ln in out.strip().splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


def test_fold_gating(policy_probe):
    """Every excluded shape, and the knob at 0, gives fold = 0 and otherwise the choice and the workspace of the same shape with
    the knob off; the qualifying shapes give fold = 1 and move no buffer."""
    excluded = [dict(nu=1), dict(nu=3), dict(form=1, tile=0), dict(form=3), dict(minv=1), dict(C=2), dict(C=12), dict(dist=1), dict(tile=0),
                dict(pip=0),                                   # a masked descriptor: pre != post
                dict(pre=0, post=0, form=2),                   # symmetric, form 2: the complex-shift plan takes it
                dict(tr=32), dict(tr=128),                     # the step kernel is written for 64-row tiles
                dict(kif=0),                                   # it builds on the init-free start
                dict(nb=4097)]                                 # more SpMV workgroups than the single-column family sums
    qualifying = [dict(), dict(form=0), dict(pre=0, post=0, form=0), dict(pre=0, post=0, form=2, kcx=0), dict(nb=7, n=1546),
                  dict(nb=1024, n=65536),
                  # past four slots of 256 partials per lane the default keeps the update launches (measured slower: every SpMV
                  # workgroup re-reduces 3 nbs partials); knob 2 folds wherever the shape allows
                  dict(nb=2345, n=300071, kfo=2), dict(nb=4096, n=262144, kfo=2)]
    excluded += [dict(nb=1025, n=65600), dict(nb=2345, n=300071), dict(nb=4097, kfo=2)]
    on = policy_probe([_line(**v) for v in excluded + qualifying])
    off = policy_probe([_line(**dict(v, kfo=0)) for v in excluded + qualifying])
    for v, a, b in zip(excluded + qualifying, on, off):
        assert b[0] == 0, v                                    # knob 0: never folded
        assert a[1:] == b[1:], (v, a, b)                       # the parent's choice, byte count and every buffer offset
        assert a[0] == (0 if v in excluded else 1), (v, a)
    # the complex-shift shape really is the other plan's
    cx = policy_probe([_line(pre=0, post=0, form=2)])[0]
    assert cx[11] == 1 and cx[0] == 0
