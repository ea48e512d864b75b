"""The head of the C == 1 tile kernels in their single-tile form, read in the compiler's assembly (no GPU).

What a workgroup waits for before it has requested its tile is a serial chain of round trips.  docs/kernels/spmm.md (round 7) states
the chain the source is written for; this test compiles csrc/spmm.hip with the build's flags and holds the emitted code to it:

  * the kernel arguments arrive in ONE batch of scalar loads with one `s_waitcnt lgkmcnt(0)`;
  * ONE more round trip carries the tile's offsets (scalar loads) and with them the skip flag and the tick (vector loads) or, in
    the step kernel, the 32-byte scalar block as a single `s_load_dwordx8`;
  * then the ids and the matrix stream go out: no wait on a vector load and no SGPR spill (`v_writelane`) in front of the first
    16-byte stream load.

`s_waitcnt lgkmcnt(0)` in front of the first `global_load`: exactly one in the plain and self-dot kernels, whose first vector loads
(skip, tick) follow the argument batch.  The step kernel has neither word (its flag and iteration come with the scalar block), so
its first vector load is an id load, whose address is made of the offsets: the compiler has to put the wait of the offsets' round
trip in front of it, and the count there is two.  In front of the first STREAM load the count is two in all five kernels."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# <PRE, 256, CBV = false, SELF, ONE = true> and <256, DS = 4, DECIDE, ONE = true>
PLAIN = [("spmv_tile_kernelILb0ELi256ELb0ELb0ELb1EEE", "plain"), ("spmv_tile_kernelILb0ELi256ELb0ELb1ELb1EEE", "self dot"),
         ("spmv_tile_kernelILb1ELi256ELb0ELb1ELb1EEE", "self dot, pre: the first launch of a solve")]
STEP = [("spmv_tile_cgstep_kernelILi256ELi4ELb0ELb1EEE", "step"), ("spmv_tile_cgstep_kernelILi256ELi4ELb1ELb1EEE", "deciding step")]


@pytest.fixture(scope="module")
def asm():
    if shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("hipcc not found")
    spec = importlib.util.spec_from_file_location("check_kblock_isa", os.path.join(ROOT, "tools", "check_kblock_isa.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    text = chk.compile_to_asm(os.path.join(ROOT, "manifold_gp_amd", "csrc", "spmm.hip"),
                              ["-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form=1"])      # csrc/build.sh
    assert text is not None, "spmm.hip did not compile"
    return text.split("\n")


def kernel(lines, mangled):
    """(instructions of the kernel, its resource comment lines)"""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_ZN\d+_GLOBAL__N_1\d+" + re.escape(mangled) + r"v.*:", l)]
    assert len(starts) == 1, (mangled, starts)
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = [l.split(";")[0].strip() for l in lines[starts[0] + 1:end]]
    body = [l for l in body if l and not l.endswith(":") and not l.startswith(".")]
    meta = {}
    for l in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|ScratchSize|NumSgprs):\s*(\d+)", l)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return body, meta


def head_facts(body):
    first_load = next(i for i, l in enumerate(body) if l.startswith("global_load"))
    first_stream = next(i for i, l in enumerate(body) if l.startswith("global_load_dwordx4"))
    head = body[:first_stream]
    # the argument batch is what stands in front of the first wait (the register pair of the argument pointer is reused later, so
    # an argument load cannot be told by its base); a second batch would show as a load too many behind it
    batch_end = head.index("s_waitcnt lgkmcnt(0)")
    assert all(l.startswith("s_load") for l in head[:batch_end] if "load" in l)
    data_loads = [l for l in head[batch_end:] if l.startswith("s_load")]
    return dict(
        waits_before_load=sum(l == "s_waitcnt lgkmcnt(0)" for l in body[:first_load]),
        waits_before_stream=sum(l == "s_waitcnt lgkmcnt(0)" for l in head),
        other_lgkm_waits=[l for l in head if l.startswith("s_waitcnt") and "lgkmcnt" in l and l != "s_waitcnt lgkmcnt(0)"],
        vm_waits=[l for l in head if l.startswith("s_waitcnt") and "vmcnt" in l],
        spills=[l for l in head if l.startswith("v_writelane")],
        data_loads=data_loads,
        later_scalar_loads=[l for l in body[first_stream:] if l.startswith("s_load")],
    )


def check_common(body, meta, name):
    f = head_facts(body)
    print(name, f, meta)
    assert f["waits_before_stream"] == 2, (name, "argument batch + offsets round trip", f)
    assert f["other_lgkm_waits"] == [], (name, f)
    assert f["vm_waits"] == [], (name, "a vector load is waited for before the stream is requested", f["vm_waits"])
    assert f["spills"] == [], (name, "SGPR spill in the head", f["spills"])
    assert meta["NumVgprs"] <= 128, (name, meta)          # 938 workgroups on 256 CUs: four per CU, 16 waves, 512 / 4 registers
    assert meta["ScratchSize"] == 0, (name, meta)
    return f


@pytest.mark.parametrize("mangled,name", PLAIN)
def test_plain_and_self_dot_heads(asm, mangled, name):
    body, meta = kernel(asm, mangled)
    f = check_common(body, meta, name)
    assert f["waits_before_load"] == 1, (name, f)
    # the offsets: tile_ptr[t], tile_ptr[t + 1] as one pair, rowptr[r0], rowptr[r1]
    assert sorted(l.split()[0] for l in f["data_loads"]) == ["s_load_dword", "s_load_dword", "s_load_dwordx2"], (name, f["data_loads"])


@pytest.mark.parametrize("mangled,name", STEP)
def test_step_heads(asm, mangled, name):
    body, meta = kernel(asm, mangled)
    f = check_common(body, meta, name)
    assert f["waits_before_load"] == 2, (name, f)         # see the module docstring: no vector load precedes the ids here
    # the offsets and the scalar block, one load.  Nothing else of the kernel comes through the scalar cache but state[5], the
    # count of finished graphs that one lane of a deciding launch reads when the whole launch leaves early (cg_mark_end_of_graph)
    assert sorted(l.split()[0] for l in f["data_loads"]) == ["s_load_dword", "s_load_dword", "s_load_dwordx2", "s_load_dwordx8"], \
        (name, f["data_loads"])
    assert all(re.match(r"s_load_dword s\d+, s\[\d+:\d+\], 0x14$", l) for l in f["later_scalar_loads"]), \
        (name, "a piece of the scalar block is fetched on its own", f["later_scalar_loads"])
    assert ("ELb1ELb1EEE" in mangled) or f["later_scalar_loads"] == [], (name, f["later_scalar_loads"])
