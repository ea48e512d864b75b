"""Guard bands and poison around caller-owned memory: the carving helper and the contract run of tests/test_gpu_memory_contract.py.

One uint8 tensor per run, the ARENA, holds every array a call sees -- inputs, outputs, in/out arrays and the workspace -- as views
with a guard of at least GUARD bytes in front of the first, between neighbours and behind the last.  The guard behind an array starts
at the byte after its last element.  Only torch and numpy: the helper works the same on CPU and device tensors, and
tests/test_guarded_cpu.py runs it against Python "entry points" that each commit one defect.

Placement `aligned`: every array starts at a multiple of 256 bytes.  `least`: at 256 k + floor, the weakest alignment the header
allows for it (Spec.floor: by default one element off a 16-byte boundary, 8 bytes off for doubles; the case states 8 / 16 for
workspaces and 0 where the header demands 16-byte alignment).

Fills: LO is all bytes 0x00, HI all bytes 0xFF (NaN as float or double, -1 as int32).  The guards take one, the workspace and the
pure outputs the other, so a stray write cannot match both and a stale read differs between the two runs.

The second half of the file is the stream-order run of tests/test_gpu_stream_order.py on the same arena (run_stream_order).
"""
import numpy as np
import torch

GUARD = 1 << 20          # 16 x the largest tile any kernel stores (128 x 128 fp32 = 64 KiB)
LO, HI = 0x00, 0xFF
PLACEMENTS = ("aligned", "least")
FILLS = ((LO, HI), (HI, LO))          # (guard fill, workspace / output fill)
ERR_WORKSPACE = -2

_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.uint8: np.uint8,
       torch.int16: np.int16, torch.int64: np.int64}


class Spec:
    __slots__ = ("name", "dtype", "numel", "role", "init", "floor", "start", "nbytes")

    def __init__(self, name, dtype, numel, role, init, floor):
        assert role in ("in", "inout", "out", "work"), role
        self.name, self.dtype, self.numel, self.role, self.init = name, dtype, int(numel), role, init
        isz = torch.empty(0, dtype=dtype).element_size()
        self.floor = (8 if isz == 8 else isz) if floor is None else int(floor)
        assert self.floor % isz == 0 and 0 <= self.floor < 256
        self.nbytes = self.numel * isz
        self.start = None


class Recorder:
    """First pass over a case: records what it carves and hands out host stand-ins of the right shape, so that the arena can be
    sized (the size queries of the library read sizes and struct fields, never device memory)."""

    def __init__(self):
        self.specs = []

    def __call__(self, name, dtype, numel, role, init=None, floor=None):
        assert all(s.name != name for s in self.specs), "array %s carved twice" % name
        if init is not None:
            init = np.ascontiguousarray(init, dtype=_NP[dtype]).reshape(-1)
            assert init.size == numel, (name, init.size, numel)
        self.specs.append(Spec(name, dtype, numel, role, init, floor))
        return torch.zeros(max(int(numel), 1), dtype=dtype)[:int(numel)]


class Arena:
    def __init__(self, specs, placement, guard_fill, body_fill, device):
        assert placement in PLACEMENTS and {guard_fill, body_fill} == {LO, HI}
        self.specs, self.placement, self.guard_fill, self.body_fill = specs, placement, guard_fill, body_fill
        cursor = 0
        for s in specs:
            start = -(-(cursor + GUARD) // 256) * 256
            if placement == "least":
                start += s.floor
            s.start = start
            cursor = start + s.nbytes
        self.size = cursor + GUARD
        raw = torch.empty(self.size + 256, dtype=torch.uint8, device=device)
        shift = (-raw.data_ptr()) % 256
        self.raw = raw
        self.mem = raw[shift:shift + self.size]
        assert self.mem.data_ptr() % 256 == 0
        self.mem.fill_(guard_fill)
        mask = np.ones(self.size, dtype=bool)
        self.views = {}
        for s in specs:
            view = self.mem[s.start:s.start + s.nbytes].view(s.dtype)
            assert view.numel() == s.numel and (s.numel == 0 or view.data_ptr() == self.mem.data_ptr() + s.start)
            if s.role in ("out", "work"):
                self.mem[s.start:s.start + s.nbytes].fill_(body_fill)
            else:
                assert s.init is not None, "input %s needs its values" % s.name
                view.copy_(torch.from_numpy(s.init.view(np.uint8)).to(device).view(s.dtype))
            mask[s.start:s.start + s.nbytes] = False
            self.views[s.name] = view
        self.guard_mask = torch.from_numpy(mask).to(device)
        self.before = self.mem.clone()

    def carve(self, name, dtype, numel, role, init=None, floor=None):
        """Second pass over a case: the same requests in the same order get the views."""
        view = self.views[name]
        assert view.dtype == dtype and view.numel() == numel, "case carved %s differently in its two passes" % name
        return view

    def spec(self, name):
        return next(s for s in self.specs if s.name == name)

    # ------------------------------------------------------------------------------------------------------------------ checks
    def check(self):
        """Per array, the guard bytes that changed around it: a list of dicts {array, side ('before' | 'after'), first, last,
        count}.  `first` / `last` are byte offsets relative to the array: for 'after' from the byte behind its last element (0 =
        the first byte past the end), for 'before' from its first byte (-1 = the byte in front of it).  A gap between two arrays
        is split in the middle: each half belongs to the nearer array.  Empty list: every guard is intact."""
        bad = (self.mem != self.guard_fill) & self.guard_mask
        if not bool(bad.any()):
            return []
        pos = torch.nonzero(bad).reshape(-1).cpu().numpy()
        out, edges = [], []
        for i, s in enumerate(self.specs):
            lo = 0 if i == 0 else (self.specs[i - 1].start + self.specs[i - 1].nbytes + s.start) // 2
            hi = self.size if i + 1 == len(self.specs) else (s.start + s.nbytes + self.specs[i + 1].start) // 2
            edges.append((s, lo, hi))
        for s, lo, hi in edges:
            for side, a, b, origin in (("before", lo, s.start, s.start), ("after", s.start + s.nbytes, hi, s.start + s.nbytes)):
                hit = pos[(pos >= a) & (pos < b)]
                if hit.size:
                    out.append(dict(array=s.name, side=side, first=int(hit[0] - origin), last=int(hit[-1] - origin),
                                    count=int(hit.size)))
        return out

    def changed(self, name):
        """Byte offsets (first, last, count) at which the array differs from its state before the call; None when unchanged."""
        s = self.spec(name)
        diff = self.mem[s.start:s.start + s.nbytes] != self.before[s.start:s.start + s.nbytes]
        if not bool(diff.any()):
            return None
        pos = torch.nonzero(diff).reshape(-1)
        return int(pos[0]), int(pos[-1]), int(pos.numel())

    def raw_bytes(self, name, numel=None):
        s = self.spec(name)
        isz = s.nbytes // s.numel if s.numel else 1
        n = s.numel if numel is None else int(numel)
        assert 0 <= n <= s.numel, "extent of %s beyond the array" % name
        return self.mem[s.start:s.start + n * isz].cpu().numpy().copy(), isz


def describe(findings):
    return "; ".join("%s: %d guard byte(s) changed %s it, offsets %+d .. %+d" % (f["array"], f["count"], f["side"], f["first"], f["last"])
                     for f in findings)


class Call:
    """What a case returns.
    run(work_bytes) -> (rc, host): makes the call(s) with the workspace size given (None: the queried size) and returns the code
        and a dict of host outputs (numpy arrays / numbers) that belong to the result; it synchronises before it returns.
    query: bytes the matching *_workspace_bytes() returns for these arguments (0: no workspace).
    extent: {output or in/out array: documented number of leading ELEMENTS, None = all of it, or a function of the host dict}.
    fill_bar / placement_bar: "bitwise", or (why, {array: tolerance per element}) where the header promises no repeatable result /
        documents another summation order on the scalar path; the tolerance is the bar of the entry point's own float64 test.
    probe: optional function run after the call that asserts the kernel family meant really ran."""

    def __init__(self, run, query=0, extent=None, fill_bar="bitwise", placement_bar="bitwise", probe=None, short_rc=ERR_WORKSPACE):
        self.run, self.query, self.extent = run, int(query), dict(extent or {})
        self.fill_bar, self.placement_bar, self.probe, self.short_rc = fill_bar, placement_bar, probe, short_rc


CHECKS = ("rc", "guards", "inputs", "fill", "placement", "extent", "short")


def _result(arena, call, host):
    res = {}
    for s in arena.specs:
        if s.role in ("out", "inout"):
            ext = call.extent.get(s.name)
            if callable(ext):
                ext = ext(host)
            res[s.name] = arena.raw_bytes(s.name, ext) + (s.dtype, s.role)
    for k, v in sorted(host.items()):
        a = np.ascontiguousarray(v)
        res["host:" + k] = (a.reshape(-1).view(np.uint8).copy(), a.itemsize, None, "host")
    return res


def _unwritten(hi_bytes, lo_bytes, isz):
    """Elements that hold the HI fill in the HI run AND the LO fill in the LO run: nobody wrote them."""
    n = min(hi_bytes.size, lo_bytes.size) // isz
    h = (hi_bytes[:n * isz].reshape(n, isz) == HI).all(axis=1)
    l = (lo_bytes[:n * isz].reshape(n, isz) == LO).all(axis=1)
    return h & l


def _compare(a, b, isz, dtype, bar, name, skip=None):
    """Indices of the elements of array `name` that differ under `bar`: bitwise, or by more than the case's per-element tolerance
    (bar = (why, {array: tolerance per element})) -- an array the bar does not name is compared bitwise.  A differing length counts
    as element -1."""
    if a.size != b.size:
        return np.array([-1])
    n = a.size // isz
    same = (a.reshape(n, isz) == b.reshape(n, isz)).all(axis=1)
    tol = None if bar == "bitwise" else bar[1].get(name)
    if tol is None:
        diff = ~same
    else:
        x, y = a.view(_NP[dtype]).astype(np.float64), b.view(_NP[dtype]).astype(np.float64)
        tol = np.broadcast_to(np.asarray(tol, np.float64).reshape(-1) if np.ndim(tol) else tol, x.shape)
        with np.errstate(invalid="ignore"):
            close = np.abs(x - y) <= tol
        diff = ~(close | same)
    if skip is not None:
        diff &= ~skip
    return np.nonzero(diff)[0]


def _bar_name(bar):
    return bar if bar == "bitwise" else bar[0]


def run_contract(case, shape, device, sync=lambda: None):
    """Runs `case` at `shape` under the four combinations {aligned, least} x FILLS, then once more with a workspace one byte
    short, and returns {check: [messages]} for the seven checks of the memory contract (CHECKS); all lists empty = the entry
    point keeps the contract at this shape."""
    rec = Recorder()
    case(rec, shape)
    found = {c: [] for c in CHECKS}
    results = {}
    for placement in PLACEMENTS:
        for gfill, bfill in FILLS:
            tag = "%s/guards %02X" % (placement, gfill)
            arena = Arena([Spec(s.name, s.dtype, s.numel, s.role, s.init, s.floor) for s in rec.specs], placement, gfill, bfill, device)
            call = case(arena.carve, shape)
            sync()
            arena.before = arena.mem.clone()
            rc, host = call.run(None)
            sync()
            if rc != 0:
                found["rc"].append("%s: returned %d" % (tag, rc))
                continue
            if call.probe is not None:
                call.probe(host)
            guards = arena.check()
            if guards:
                found["guards"].append("%s: %s" % (tag, describe(guards)))
            for s in arena.specs:
                if s.role == "in":
                    ch = arena.changed(s.name)
                    if ch:
                        found["inputs"].append("%s: const input %s changed at byte offsets %d .. %d (%d bytes)" % ((tag, s.name) + ch))
            results[(placement, bfill)] = (_result(arena, call, host), call)
            del arena
    # 6 then 4: entries nobody wrote are reported once, as `extent`; every other difference between the fills as `fill`
    unwritten = {}
    for placement in PLACEMENTS:
        if (placement, HI) not in results or (placement, LO) not in results:
            continue
        (rh, call), (rl, _) = results[(placement, HI)], results[(placement, LO)]
        for name in rh:
            bh, isz, dtype, role = rh[name]
            bl = rl[name][0]
            skip = None
            if role == "out" and bh.size == bl.size:
                skip = _unwritten(bh, bl, isz)
                unwritten[(placement, name)] = skip
                if skip.any():
                    idx = np.nonzero(skip)[0]
                    found["extent"].append("%s: %s holds its fill inside the documented extent at %d element(s), first %d, last %d"
                                           % (placement, name, idx.size, idx[0], idx[-1]))
            idx = _compare(bh, bl, isz, dtype, call.fill_bar, name, skip)
            if idx.size:
                found["fill"].append("%s: %s moves with the fill of workspace / outputs at %d element(s), first %d, last %d (bar: %s)"
                                     % (placement, name, idx.size, idx[0], idx[-1], _bar_name(call.fill_bar)))
    for bfill in (HI, LO):
        if ("aligned", bfill) not in results or ("least", bfill) not in results:
            continue
        (ra, call), (rl, _) = results[("aligned", bfill)], results[("least", bfill)]
        for name in ra:
            ba, isz, dtype, role = ra[name]
            skip = None
            if ("aligned", name) in unwritten and ("least", name) in unwritten and ba.size == rl[name][0].size:
                skip = unwritten[("aligned", name)] | unwritten[("least", name)]
            idx = _compare(ba, rl[name][0], isz, dtype, call.placement_bar, name, skip)
            if idx.size:
                found["placement"].append("body fill %02X: %s differs between aligned and least placement at %d element(s), first %d, "
                                          "last %d (bar: %s)" % (bfill, name, idx.size, idx[0], idx[-1], _bar_name(call.placement_bar)))
    # 7: one byte short
    gfill, bfill = FILLS[0]
    arena = Arena([Spec(s.name, s.dtype, s.numel, s.role, s.init, s.floor) for s in rec.specs], "aligned", gfill, bfill, device)
    call = case(arena.carve, shape)
    if call.query > 0:
        sync()
        arena.before = arena.mem.clone()
        rc, _ = call.run(call.query - 1)
        sync()
        if rc != call.short_rc:
            found["short"].append("work_bytes = query - 1 = %d returned %d, not %d" % (call.query - 1, rc, call.short_rc))
        guards = arena.check()
        if guards:
            found["short"].append("short workspace: " + describe(guards))
        for s in arena.specs:
            ch = arena.changed(s.name)
            if ch:
                found["short"].append("short workspace: %s (%s) was touched at byte offsets %d .. %d (%d bytes)" % ((s.name, s.role) + ch))
    return found


def report(found):
    return "\n".join("[%s] %s" % (c, m) for c in CHECKS for m in found[c])


# ======================================================================================================================================
# Stream order (tests/test_gpu_stream_order.py, docs/stream_contract.md): the same case, run on a side stream behind pending work.
#
# The arena is put into a DECOY state -- every float input rolled by one element, indices / masks / sizes true, workspace and outputs
# zero -- and the side stream gets, in this order: a bounded delay, one copy of the TRUE image over the whole arena, the case.  A
# launch on the side stream sees the true inputs.  A launch issued on any other stream runs while the delay is pending: it reads the
# decoy (valid values at true addresses, so a wrong number and never a wrong address), and whatever it writes is wiped by the image
# copy.  At every inner sync of a sequence the arena is re-armed, so each step runs behind pending work.
ORDER_CHECKS = ("rc", "guards", "inputs", "order", "window")
DELAY_CAP_MS = 200.0
DELAY_FLOOR_MS = 10.0     # twice the smallest of 5 / 10 / 20 / 50 ms at which every control was reported 10 times out of 10: measured,
                          # docs/stream_contract.md.  The delay of a run is max(20 x its default-stream duration, this), capped
_FLOATS = (torch.float32, torch.float64)


def carries_decoy(spec):
    return spec.role in ("in", "inout") and spec.dtype in _FLOATS


def decoy_image(specs, true_bytes):
    """The decoy state of an arena whose true bytes are `true_bytes` (uint8 numpy, arena.mem): a copy in which every float32 /
    float64 array of role in / inout holds its values rolled by one element.  Integer and uint8 arrays, guards, workspace and outputs
    stay as they are.  Returns (image, names of the arrays that differ from their decoy, names of the float inputs that do not: a
    constant array has no decoy)."""
    image = np.array(true_bytes, dtype=np.uint8, copy=True)
    differ, constant = [], []
    for s in specs:
        if not carries_decoy(s) or s.numel == 0:
            continue
        cur = image[s.start:s.start + s.nbytes].view(_NP[s.dtype])
        rolled = np.roll(cur, 1)
        (constant if rolled.tobytes() == cur.tobytes() else differ).append(s.name)
        image[s.start:s.start + s.nbytes] = rolled.view(np.uint8)
    return image, differ, constant


class sync_hook:
    """`with sync_hook(owner, fn):` makes owner.SYNC_HOOK = fn (owner: tests/_entry_cases.py, whose _sync() calls it behind every
    device sync) and puts back what was there before, also when the body raises."""

    def __init__(self, owner, fn):
        self.owner, self.fn = owner, fn

    def __enter__(self):
        self.keep = self.owner.SYNC_HOOK
        self.owner.SYNC_HOOK = self.fn
        return self

    def __exit__(self, *exc):
        self.owner.SYNC_HOOK = self.keep
        return False


class Delay:
    """A bounded stretch of device time on the current stream: torch.cuda._sleep, calibrated once against events; a chain of
    matmuls where this torch build cannot spin.  Never a gate the host releases: a test that died would leave the stream waiting."""

    def __init__(self, device):
        try:
            torch.cuda._sleep(1000)
            self.unit = lambda k: torch.cuda._sleep(int(k))
            self.kind, probe = "torch.cuda._sleep", 1 << 24
        except (AttributeError, RuntimeError):
            a = torch.ones(1024, 1024, device=device)
            b, c = a.clone(), a.clone()

            def chain(k):
                for _ in range(int(k)):
                    torch.mm(a, b, out=c)
            self.unit, self.kind, probe = chain, "matmul chain", 64
        self.unit(probe // 8)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        self.unit(probe)
        t1.record()
        t1.synchronize()
        self.per_ms = probe / max(t0.elapsed_time(t1), 1e-3)

    def enqueue(self, ms):
        self.unit(max(1, int(ms * self.per_ms)))


def window_open(delay, ms, between=lambda: None):
    """On the current (side) stream: enqueues a delay of `ms`, an event behind it and whatever `between` enqueues; then a marker op
    on the default stream.  True when the marker completed while the event was still unsignalled: work on the default stream
    overtakes the side stream for the length of the delay."""
    dev = torch.cuda.current_stream().device
    delay.enqueue(ms)
    ev = torch.cuda.Event()
    ev.record()
    between()
    with torch.cuda.stream(torch.cuda.default_stream(dev)):
        torch.zeros(1, device=dev).add_(1.0)
        done = torch.cuda.Event()
        done.record()
    done.synchronize()
    return not ev.query(), ev


def side_stream(device, delay, tries=8, probe_ms=2.0):
    """A fresh torch.cuda.Stream that does not wait for the default stream, nor the default stream for it.  The runtime maps its
    streams onto a few hardware queues, and two streams that land on one queue run in issue order: behind such a stream nothing is
    pending from the default stream's point of view, and work issued there by mistake is ordered all the same.  So a new stream is
    probed with a short delay and dropped for the next one when the marker does not overtake it (one stream alive at a time)."""
    side = None
    for _ in range(tries):
        side = None                                    # (drop the last one before the next is made)
        side = torch.cuda.Stream(device)
        with torch.cuda.stream(side):
            ok, _ = window_open(delay, probe_ms)
        side.synchronize()
        if ok:
            break
    return side


def _differing(name, idx, what):
    return "%s: %s at %d element(s), first %d, last %d" % (name, what, idx.size, idx[0], idx[-1])


def run_stream_order(case, shape, device, owner, delay, floor_ms=None):
    """Runs `case` at `shape` once on the default stream and once on a fresh side stream behind a delay (see above; `owner` is the
    module whose SYNC_HOOK re-arms the arena at the inner syncs, `delay` a Delay).  Returns ({check: [messages]} for ORDER_CHECKS,
    info): `order` = the side-stream result differs from the default-stream one under the case's fill_bar; `window` = a marker on
    the default stream did not complete while the delay was still pending, so the run proves nothing.  info: decoys (arrays that
    differ from their decoy), constant (float inputs that do not), rearms, delay_ms, ref_ms."""
    floor_ms = DELAY_FLOOR_MS if floor_ms is None else floor_ms
    rec = Recorder()
    case(rec, shape)
    fresh = lambda: Arena([Spec(s.name, s.dtype, s.numel, s.role, s.init, s.floor) for s in rec.specs], "aligned", HI, LO, device)
    found = {c: [] for c in ORDER_CHECKS}
    info = dict(decoys=0, constant=[], rearms=0, delay_ms=0.0, ref_ms=0.0)
    # 1. the reference: default stream, nothing pending
    arena = fresh()
    call = case(arena.carve, shape)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    rc, host = call.run(None)
    t1.record()
    t1.synchronize()
    info["ref_ms"] = t0.elapsed_time(t1)
    if rc != 0:
        found["rc"].append("default stream: returned %d" % rc)
        return found, info
    if call.probe is not None:
        call.probe(host)
    ref = _result(arena, call, host)
    del arena, call
    # 2. the second arena, its true image and its decoy state
    arena = fresh()
    case(arena.carve, shape)
    torch.cuda.synchronize()
    true = arena.mem.clone()
    image, differ, constant = decoy_image(arena.specs, true.cpu().numpy())
    info["decoys"], info["constant"] = len(differ), constant
    arena.mem.copy_(torch.from_numpy(image).to(device))
    torch.cuda.synchronize()
    info["delay_ms"] = ms = min(DELAY_CAP_MS, max(20.0 * info["ref_ms"], floor_ms))
    # 3. / 4. the side-stream run
    side = side_stream(device, delay)
    state = {}

    def arm(restore):
        """On the side stream: delay, then `restore` over the arena; the marker on the default stream checks the window."""
        state["restore"] = restore                       # alive until the copy has run
        ok, state["ev"] = window_open(delay, ms, lambda: arena.mem.copy_(restore))
        if not ok:
            found["window"].append("arm %d: the delay of %.1f ms had run out before a marker on the default stream completed"
                                   % (info["rearms"], ms))

    def rearm():
        """Behind a device sync: keep what the arena holds, roll the float inputs, then delay + restore on the side stream."""
        snap = arena.mem.clone()
        for s in arena.specs:
            if carries_decoy(s) and s.numel:
                arena.views[s.name].copy_(torch.roll(snap[s.start:s.start + s.nbytes].view(s.dtype), 1))
        torch.cuda.synchronize()
        info["rearms"] += 1
        arm(snap)

    try:
        with torch.cuda.stream(side):
            arm(true)
            with sync_hook(owner, rearm):
                call = case(arena.carve, shape)
                if state["ev"].query():              # building the case waited for the device: the delay is spent, arm again
                    torch.cuda.synchronize()
                    rearm()
                rc, host = call.run(None)
    finally:
        torch.cuda.synchronize()
    if rc != 0:
        found["rc"].append("side stream: returned %d" % rc)
        return found, info
    guards = arena.check()
    if guards:
        found["guards"].append("side stream: %s" % describe(guards))
    arena.before = true
    for s in arena.specs:
        if s.role == "in":
            ch = arena.changed(s.name)
            if ch:
                found["inputs"].append("side stream: const input %s changed at byte offsets %d .. %d (%d bytes)" % ((s.name,) + ch))
    got = _result(arena, call, host)
    for name in ref:
        a, isz, dtype, _ = ref[name]
        idx = _compare(a, got[name][0], isz, dtype, call.fill_bar, name)
        if idx.size:
            found["order"].append(_differing(name, idx, "differs between the default stream and the side stream (bar: %s)"
                                             % _bar_name(call.fill_bar)))
    return found, info


def report_order(found):
    return "\n".join("[%s] %s" % (c, m) for c in ORDER_CHECKS for m in found[c])
