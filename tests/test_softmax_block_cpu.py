"""The block softmax solver, host side (no GPU): the layout header manifold_gp_amd/csrc/softmax_block.h compiled with a host
compiler and probed -- the contracts are stated from the indexing of the three kernels of csrc/softmax_cg_block.hip, emulated
here --, the four C entry points and their argument checks, the validation of the Python wrappers on host tensors, and the
float64 restatement of the block recurrence (tests/_softmax_block_ref.py) against the exact dense solve."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _softmax_block_ref as bref
import _softmax_ref as sref
from test_softmax_cpu import _fake_desc, _op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
needs_cxx = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

NS = (1, 63, 64, 65, 257, 1546, 70000)
SHAPES = ((2, 1), (2, 128), (3, 5), (3, 85), (10, 16), (10, 25), (16, 16), (17, 15), (33, 7), (64, 1), (64, 4))     # (C, S)

PROBE = r"""
#include <stdio.h>
#include <sys/mman.h>
#include <vector>
#include "softmax_block.h"

int main(void) {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'k') {
      printf("K %d %d %d %d %d %zu %zu\n", (int)kBlkThreads, (int)kBlkMaxCols, (int)kBlkMaxClasses, (int)kBlkHessMaxBlocks,
             (int)kBlkUpdateMaxBlocks, sizeof(SblkHead), sizeof(SblkSample));
    } else if (cmd == 'o') {            // shape_ok: C S
      int C, S; if (scanf("%d %d", &C, &S) != 2) return 1;
      printf("O %d\n", sblk_shape_ok(C, S) ? 1 : 0);
    } else if (cmd == 'h') {            // the plans: n C S
      long long n; int C, S; if (scanf("%lld %d %d", &n, &C, &S) != 3) return 1;
      const SblkHess h = sblk_hess(n, C, S);
      const SblkUpdate u = sblk_update(n, C, S);
      printf("H %d %d %d %lld %lld %lld %d %lld %zu\n", h.tc, h.rows_per_block, h.grid, (long long)h.stride, (long long)h.node_step,
             (long long)h.passes, u.grid, (long long)u.stride, sblk_partial_doubles(S));
    } else if (cmd == 'g') {            // sblk_group: n C S b g
      long long n; int C, S, b, g; if (scanf("%lld %d %d %d %d", &n, &C, &S, &b, &g) != 5) return 1;
      printf("G %lld\n", (long long)sblk_group(sblk_hess(n, C, S), b, g));
    } else if (cmd == 'w') {            // the writers and the readers of the partials, as the kernels index them: n C S
      long long n; int C, S; if (scanf("%lld %d %d", &n, &C, &S) != 3) return 1;
      const SblkHess h = sblk_hess(n, C, S);
      // (a) inside a workgroup: thread t < S adds the groups first_group(b, t), + S, ... < rows_per_block
      long long bad_group = 0;
      std::vector<int> taken(h.rows_per_block);
      for (int b = 0; b < h.grid; ++b) {
        for (int& v : taken) v = 0;
        for (int t = 0; t < S; ++t)
          for (int gg = sblk_first_group(h, S, b, t); gg < h.rows_per_block; gg += S) {
            if (gg < 0 || sblk_group(h, b, gg) % S != t) ++bad_group;
            else ++taken[gg];
          }
        for (int v : taken) if (v != 1) ++bad_group;
      }
      // (b) the slots: workgroup b writes slot (t, b, grid) for t < S; the reduce reads slot (s, k, grid) for k < grid
      std::vector<int> writes(sblk_partial_doubles(S) / 2, 0);
      long long out_of_range = 0, bad_read = 0;
      for (int b = 0; b < h.grid; ++b)
        for (int t = 0; t < S; ++t) {
          const size_t at = sblk_slot(t, b, h.grid);
          if (at % 2 || at + 2 > sblk_partial_doubles(S)) ++out_of_range; else ++writes[at / 2];
        }
      for (int s = 0; s < S; ++s)
        for (int k = 0; k < h.grid; ++k) {
          const size_t at = sblk_slot(s, k, h.grid);
          if (at % 2 || at + 2 > sblk_partial_doubles(S) || writes[at / 2] != 1) ++bad_read;
        }
      printf("W %lld %lld %lld\n", bad_group, out_of_range, bad_read);
    } else if (cmd == 'v') {            // the carve: n C S opbytes
      long long n; int C, S; size_t opbytes; if (scanf("%lld %d %d %zu", &n, &C, &S, &opbytes) != 4) return 1;
      MgpArena count;
      SblkCarve nb;
      sblk_carve(count, n, C, S, opbytes, &nb);
      const bool count_null = !nb.R && !nb.P && !nb.Sv && !nb.W && !nb.partials && !nb.sums && !nb.state && !nb.opwork;
      const size_t counted = count.off;
      char* base = (char*)mmap(nullptr, counted, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
      if (base == (char*)MAP_FAILED) return 1;
      MgpArena ar(base, counted), tight(base, counted - 1);
      SblkCarve b, t;
      const bool ok = sblk_carve(ar, n, C, S, opbytes, &b);
      const bool short_ok = sblk_carve(tight, n, C, S, opbytes, &t);
      const void* p[] = {b.R, b.P, b.Sv, b.W, b.partials, b.sums, b.state, b.opwork};
      printf("V %zu %zu %d %d %d %zu", counted, ar.off, ok ? 1 : 0, short_ok ? 1 : 0, count_null ? 1 : 0, sblk_state_bytes(S));
      for (const void* q : p) printf(" %lld", q ? (long long)((const char*)q - base) : -1LL);
      MgpArena hc;
      double* hp;
      sblk_carve_hess(hc, S, &hp);
      printf(" %zu\n", hc.off);
      munmap(base, counted);
    } else return 1;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("softmax_block")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "manifold_gp_amd", "csrc"), str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.check_output([str(exe)], input="\n".join(lines) + "\n", text=True)
        rows = [ln.split() for ln in out.strip().splitlines()]
        assert len(rows) == len(lines), (len(rows), len(lines))
        return rows
    return run


@pytest.fixture(scope="module")
def K(probe):
    t = probe(["k"])[0]
    names = ("threads", "max_cols", "max_classes", "hess_cap", "update_cap", "head_bytes", "sample_bytes")
    k = dict(zip(names, (int(v) for v in t[1:])))
    # the kernels are written for 256-thread workgroups of four waves; the Python layer states the same column cap
    assert k["threads"] == 256 and k["max_cols"] == 256 and k["max_classes"] == 64, k
    return k


def _plan(probe, n, C, S):
    t = probe(["h %d %d %d" % (n, C, S)])[0]
    names = ("tc", "rows", "grid", "stride", "node_step", "passes", "ugrid", "ustride", "partial_doubles")
    return dict(zip(names, (int(v) for v in t[1:])))


# ------------------------------------------------------------------------------------------------ 1: the layout
@needs_cxx
def test_shape_limits(probe, K):
    for C, S in SHAPES:
        assert probe(["o %d %d" % (C, S)])[0] == ["O", "1"], (C, S)
    for C, S in ((1, 4), (65, 1), (3, 0), (3, -1), (3, 86), (2, 129), (64, 5), (10, 26), (0, 1)):
        assert probe(["o %d %d" % (C, S)])[0] == ["O", "0"], (C, S)


@needs_cxx
@pytest.mark.parametrize("C, S", SHAPES)
def test_every_row_has_one_lane_group_and_every_slot_one_writer(probe, K, C, S):
    """The epilogue, from sblk_hess_kernel's indexing: lane l of workgroup b is lane l % tc of group g = l / tc, the group has the
    launch-wide index j = sblk_group(b, g), the sample j % S and, at pass k < passes, the node j / S + k node_step; it is live where
    that node is < n.  (a) tc is a power of two >= C that divides the wave, so no group straddles one, and the workgroup's
    groups fill it; (b) every (node, sample) row is live in exactly one (group, pass); (c) the groups of one pass of a workgroup
    take consecutive rows; (d) inside a workgroup every group is added into the sum of its own sample exactly once, every slot
    the reduce reads lies inside the buffer and has exactly one writer; (e) the grid is within its cap.
    The update, from sblk_update_kernel's: thread t of workgroup b takes the elements e = b 256 + t + m stride; its sample
    (e / C) % S must not depend on m, and the elements < n S C are each taken once."""
    for n in NS:
        p = _plan(probe, n, C, S)
        tc, rows, grid = p["tc"], p["rows"], p["grid"]
        assert tc >= C and tc < 2 * C and tc & (tc - 1) == 0 and 64 % tc == 0 and rows * tc == K["threads"], p
        assert 1 <= grid <= K["hess_cap"] and p["stride"] == grid * rows, p
        # sblk_group is what the kernel calls: spot-check it against b rows + g at the corners
        for b, g in ((0, 0), (grid - 1, rows - 1), (grid // 2, rows // 2)):
            assert int(probe(["g %d %d %d %d %d" % (n, C, S, b, g)])[0][1]) == b * rows + g
        j = np.arange(grid * rows, dtype=np.int64)
        k = np.arange(p["passes"], dtype=np.int64)
        node = (j // S)[None, :] + k[:, None] * p["node_step"]
        live = node < n
        row = (node * S + (j % S)[None, :])[live]
        assert row.size == n * S and np.array_equal(np.sort(row), np.arange(n * S)), (n, C, S)
        # consecutive rows within a workgroup's pass (the loads of a wave stay contiguous)
        first = node[0] * S + j % S
        assert np.array_equal(np.diff(first.reshape(grid, rows), axis=1), np.ones((grid, rows - 1), np.int64)), (n, C, S)
        assert probe(["w %d %d %d" % (n, C, S)])[0] == ["W", "0", "0", "0"], (n, C, S)
        assert p["partial_doubles"] >= 2 * S * grid
        ug, us = p["ugrid"], p["ustride"]
        assert 1 <= ug <= K["update_cap"] and us == ug * K["threads"] and us % (S * C) == 0, p
        # a multiple of S C keeps (e / C) % S: checked on the elements themselves for the first threads of the last workgroup
        e = (ug - 1) * K["threads"] + np.arange(min(K["threads"], 64), dtype=np.int64)
        for m in (1, 2, 7):
            assert np.array_equal((e // C) % S, ((e + m * us) // C) % S)
        # no needless workgroups beyond one unit of the grid's granularity
        assert (grid - 1) * rows < n * S + (S // np.gcd(S, rows)) * rows
        assert (ug - 1) * K["threads"] < n * S * C + (S * C // np.gcd(S * C, K["threads"])) * K["threads"]


@needs_cxx
@pytest.mark.parametrize("C, S", SHAPES)
def test_counting_and_real_arena_agree(probe, K, C, S):
    """A counting arena and a real one over exactly the counted bytes hand out the same layout; one byte less fails; every
    buffer is 16-byte aligned, inside the workspace and disjoint from the others at the size its kernel indexes."""
    for n in NS:
        for opbytes in (0, 1000, 4 * n * S * C):
            t = probe(["v %d %d %d %d" % (n, C, S, opbytes)])[0]
            counted, real, ok, short_ok, count_null, state_bytes = (int(v) for v in t[1:7])
            offs = [int(v) for v in t[7:15]]
            assert counted == real and ok == 1 and short_ok == 0 and count_null == 1, t
            assert state_bytes == K["head_bytes"] + S * K["sample_bytes"]
            plan = _plan(probe, n, C, S)
            sizes = [4 * n * S * C] * 4 + [8 * 2 * S * plan["grid"], 8 * 2 * S, state_bytes, opbytes]
            spans = sorted((o, o + sz) for o, sz in zip(offs, sizes))
            assert all(o >= 0 and o % 16 == 0 for o in offs), offs
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= counted, spans
            assert int(t[15]) >= 8 * 2 * S * plan["grid"]                        # the epilogue's own workspace


# ------------------------------------------------------------------------------------------------ 2: the entry points
NEW = ("mgp_softmax_cg_block_workspace_bytes", "mgp_softmax_cg_block", "mgp_softmax_hessian_add_block_workspace_bytes",
       "mgp_softmax_hessian_add_block")


def test_signatures_name_the_entry_points_and_the_library_exports_them():
    from manifold_gp_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "mgp_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert name + "(" in header
        assert hasattr(handle, name)


def test_block_solver_checks_its_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    op, keep = _op()
    ref = ctypes.byref(op)
    buf = (ctypes.c_float * (1 << 20))()
    u = (ctypes.addressof(buf) + 15) // 16 * 16
    wb = lib.mgp_softmax_cg_block_workspace_bytes
    need = wb(ref, 3, 5)
    assert need >= 4 * 15 * 4 + 16 * 5 + lib.mgp_operator_workspace_bytes(ref, 15) and need <= 1 << 21
    assert wb(None, 3, 5) == 0 and wb(ref, 1, 5) == 0 and wb(ref, 65, 1) == 0 and wb(ref, 3, 0) == 0 and wb(ref, 3, 86) == 0
    assert wb(ref, 64, 4) > 0 and wb(ref, 64, 5) == 0 and wb(ref, 2, 128) > 0 and wb(ref, 2, 129) == 0
    cg = lib.mgp_softmax_cg_block
    ok = dict(op=ref, pi=u, C=3, S=5, B=u, X=u + 64, tol=1e-3, max_iter=10, check=8, work=u + 256, wb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return cg(a["op"], a["pi"], a["C"], a["S"], a["B"], a["X"], a["tol"], a["max_iter"], a["check"], None, None, None,
                  a["work"], a["wb"], None)
    for name in ("op", "pi", "B", "X"):
        assert call(**{name: None}) == -1, name
    assert call(X=u) == -1 and call(C=1) == -1 and call(C=65) == -1 and call(S=0) == -1 and call(S=-3) == -1 and call(S=86) == -1
    assert call(C=64, S=5) == -1 and call(tol=-1.0) == -1 and call(tol=float("nan")) == -1
    assert call(max_iter=0) == -1 and call(check=-1) == -1
    assert call(work=None) == -2 and call(wb=need - 1) == -2 and call(work=u + 260) == -2
    for form in (1, 2, 3):
        bad, keep2 = _op(form)
        bad.obs_w = u
        assert wb(ctypes.byref(bad), 3, 5) == 0
        assert call(op=ctypes.byref(bad)) == -3, form
    op.nu = 0
    assert wb(ref, 3, 5) == 0 and call() == -1                            # an invalid operator


def test_block_epilogue_checks_its_arguments_without_a_device():
    from manifold_gp_amd import _lib
    lib = _lib.lib()
    buf, dbl = (ctypes.c_float * 4096)(), (ctypes.c_double * 8192)()
    u = (ctypes.addressof(buf) + 15) // 16 * 16
    d = (ctypes.addressof(dbl) + 15) // 16 * 16
    wb = lib.mgp_softmax_hessian_add_block_workspace_bytes
    need = wb(4, 3, 5)
    assert need >= 8 * 2 * 5 and wb(0, 3, 5) == 0 and wb(4, 1, 5) == 0 and wb(4, 65, 1) == 0 and wb(4, 3, 0) == 0
    assert wb(4, 3, 86) == 0 and wb(4, 64, 5) == 0 and wb(2 ** 40, 3, 85) > 0
    hess = lib.mgp_softmax_hessian_add_block
    ok = dict(pi=u, X=u, n=4, C=3, S=5, Y=u + 1024, sums=d, work=d + 256, wb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return hess(a["pi"], a["X"], a["n"], a["C"], a["S"], a["Y"], a["sums"], a["work"], a["wb"], None)
    for name in ("pi", "X", "Y"):
        assert call(**{name: None}) == -1, name
    assert call(Y=u) == -1 and call(n=0) == -1 and call(C=1) == -1 and call(C=65) == -1 and call(S=0) == -1 and call(S=86) == -1
    assert call(work=None) == -2 and call(wb=need - 1) == -2 and call(work=d + 260) == -2


# ------------------------------------------------------------------------------------------------ 3: the wrappers
def test_block_wrapper_checks_its_arguments_on_host_tensors():
    from manifold_gp_amd.classification import softmax_cg_solve_block
    d = _fake_desc()
    pi, rhs = torch.zeros(3, 3), torch.zeros(3, 4, 3)
    with pytest.raises(NotImplementedError):
        softmax_cg_solve_block(_fake_desc(form=2), pi, rhs)
    with pytest.raises(ValueError, match="pi"):
        softmax_cg_solve_block(d, torch.zeros(4, 3), torch.zeros(4, 4, 3))
    with pytest.raises(ValueError, match="num_classes"):
        softmax_cg_solve_block(d, torch.zeros(3, 1), torch.zeros(3, 4, 1))
    for bad in (torch.zeros(3, 3), torch.zeros(3, 4, 2), torch.zeros(2, 4, 3), torch.zeros(3, 0, 3), torch.zeros(3, 4, 3, 1)):
        with pytest.raises(ValueError, match="rhs"):
            softmax_cg_solve_block(d, pi, bad)
    with pytest.raises(ValueError, match="limit is 256"):
        softmax_cg_solve_block(d, pi, torch.zeros(3, 86, 3))
    with pytest.raises(ValueError, match="max_iter"):
        softmax_cg_solve_block(d, pi, rhs, max_iter=0)
    with pytest.raises(ValueError, match="check_every"):
        softmax_cg_solve_block(d, pi, rhs, check_every=0)
    with pytest.raises(ValueError, match="tol"):
        softmax_cg_solve_block(d, pi, rhs, tol=-1.0)
    with pytest.raises(ValueError, match="tol"):
        softmax_cg_solve_block(d, pi, rhs, tol=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        softmax_cg_solve_block(d, pi, rhs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        softmax_cg_solve_block(d, pi, torch.zeros(3, 85, 3))              # 255 columns: inside the limit


def _host_fit():
    from manifold_gp_amd.classification import MulticlassLaplaceFit
    z = torch.zeros(3, 3)
    return MulticlassLaplaceFit(_fake_desc(), torch.zeros(3, dtype=torch.int32), None, z, z.clone(), True, 0, [], 0.0)


def test_block_argument_of_the_fit_is_validated():
    fit = _host_fit()
    calls = (lambda b: fit.latent_samples(4, seed=1, block=b), lambda b: fit.predict_proba(4, seed=1, block=b),
             lambda b: fit.latent_variance(4, seed=1, block=b))
    for call in calls:
        for bad in (0, -1, True, 2.5, "4", 86):
            with pytest.raises(ValueError, match="block"):
                call(bad)
        with pytest.raises(ValueError, match="limit is 256"):
            call(86)
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(85)                                                      # 255 columns: valid, but host tensors
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(2)
    with pytest.raises(ValueError, match="S must be"):
        fit.latent_variance(0, seed=1, block=2)


# ------------------------------------------------------------------------------------------------ 4: the restatement
def _small_system(n=40, C=3, S=4, seed=3):
    rng = np.random.default_rng(seed)
    L = np.diag(np.full(n, 2.0)) - np.diag(np.ones(n - 1), 1) - np.diag(np.ones(n - 1), -1)
    L[0, -1] = L[-1, 0] = -1.0
    Q = 0.3 * np.eye(n) + L + 0.1 * L @ L
    obs = rng.random(n) < 0.3
    Pi = np.where(obs[:, None], sref.softmax(rng.standard_normal((n, C)) * 2.0), 0.0)
    B = rng.standard_normal((n, S, C))
    B[:, 1] = 0.0
    B[:, 2] *= 1e-3                                                       # scale does not matter to a relative residual
    return Q, obs, Pi, B


def test_block_recurrence_solves_every_sample_and_freezes_them():
    """The float64 block recurrence against the exact dense solve (_softmax_ref.Solver.solve): every sample to 1e-10 of the
    solution's largest entry; a frozen sample does not change afterwards; the zero sample takes no update."""
    Q, obs, Pi, B = _small_system()
    n, S, C = B.shape
    X, iters, rel, status, frozen_at = bref.block_cg(Q, Pi, B, 1e-13)
    solver = sref.Solver(Q, obs)
    assert status == 1 and (rel <= 1e-13).all()
    for s in range(S):
        want = solver.solve(Pi, B[:, s])
        assert np.abs(X[:, s] - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), s
        step, snap = frozen_at[s]
        assert np.array_equal(snap, X[:, s]), s
        assert iters[s] == step - 1, (s, iters[s], step)
    assert iters[1] == 0 and not X[:, 1].any() and rel[1] == 0.0
    assert len(set(int(k) for k in iters)) > 2                            # the samples stop at steps of their own
    # a sample's path does not depend on its neighbours: alone in a block of one it gives the same numbers (to rounding:
    # the dense product of numpy sums in another order at another width)
    for s in (0, 3):
        X1, it1, rel1, _, _ = bref.block_cg(Q, Pi, B[:, s:s + 1], 1e-13)
        assert np.abs(X1[:, 0] - X[:, s]).max() <= 1e-12 * np.abs(X[:, s]).max() and abs(it1[0] - iters[s]) <= 1
    # ... and equals CG on the naive dense matrix of that sample's system to rounding
    A = sref.dense_system(Q, Pi)
    x, k = bref.plain_cg(A, B[:, 0].reshape(-1), 1e-13)
    assert abs(k - iters[0]) <= 2 and np.abs(x.reshape(n, C) - X[:, 0]).max() <= 1e-10
    # max_iter: status 2, no sample beyond it
    X5, it5, rel5, st5, _ = bref.block_cg(Q, Pi, B, 1e-13, max_iter=5)
    assert st5 == 2 and it5.max() == 5 and it5[1] == 0 and np.isfinite(X5).all()
    # the block apply is the dense matrix sample by sample
    V = np.random.default_rng(0).standard_normal((n, S, C))
    W = bref.apply_block(Q, Pi, V)
    for s in range(S):
        assert np.abs(W[:, s].reshape(-1) - A @ V[:, s].reshape(-1)).max() <= 1e-12
