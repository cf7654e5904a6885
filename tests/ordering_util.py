"""DESIGN.md 4.9 ("Ordering: who waits for whom") as data, and the tools that pin it on the device.

The table: every ordered pair (A, B) of the operations below has one entry — does B, enqueued on one stream, wait for A,
enqueued earlier on another?  The entries are derived from the three rules of 4.9, not typed cell by cell.

The gate: a spin kernel of bounded, measured duration (torch.cuda._sleep) enqueued ahead of A.  While it spins A cannot
finish, so "B waits for A" and "B does not wait for A" become observable facts instead of a race that A always wins at
test sizes: B's event is still unset while the gate is closed, or it is set while the gate is closed.  Every observation
reads the gate's own event AFTERWARDS: an observation made when the gate had already opened is void, never a pass.

The control: streams share a handful of hardware queues, and two streams of one queue serialise with no help from the
library.  pick_streams() therefore chooses, from at most 8 torch streams, three that are independent of each other AND of
the streams the context itself owns (the mesh kernel's aux stream, the per-device streams of a multi-device context), by
the same observation: a trivial operation on one completes while a gate — with a frame behind it — is closed on another.

The first part of the file (the table) imports nothing but the standard library and is checked by
tests/test_ordering_util_cpu.py; the rest needs torch and a device."""
import collections
import itertools
import time

import numpy as np

# ---- the operations -----------------------------------------------------------------------------------------------------
FRAME_LIKE = ("frame", "aov")                               # share d_records, the screen masks
READERS = ("query", "shade", "radiance")                    # the families of wait_scene_readers
EDITS = ("update", "replace", "pose", "pose_skin")          # *_device entries; all record ev_upd
PLANE_CALLS = ("filter", "accumulate")                      # read no scene: their own family only
OPS = FRAME_LIKE + READERS + EDITS + PLANE_CALLS

KIND = {}
for _ops, _kind in ((FRAME_LIKE, "frame_like"), (READERS, "reader"), (EDITS, "edit")):
    for _op in _ops:
        KIND[_op] = _kind
KIND["filter"], KIND["accumulate"] = "filter", "accumulate"

# The rules of 4.9: the kind of B -> the kinds of A it waits for.  (Nothing waits for a filter or an accumulate call but the
# next call of the same family.)
WAITS_FOR = {
    "frame_like": ("frame_like", "edit"),                   # launch_frame, enqueue_aov: ev1, wait_aov, wait_scene
    "reader": ("edit", "reader"),                           # reader_begin: wait_scene, wait_scene_readers
    "edit": ("frame_like", "reader", "edit"),               # update_begin: ev1, wait_scene_readers, wait_aov, wait_scene
    "filter": ("filter",),                                  # enqueue_filter: filter.ev
    "accumulate": ("accumulate",),                          # enqueue_accumulate: accum.ev
}

# waits: B waits for A.  how: "gate" — observed behind a gate and pinned by the data; "data" — edit -> edit on two streams, the
# one cell the gate cannot reach (every Z that holds A also holds B): the final scene is the second edit's.
Expect = collections.namedtuple("Expect", "waits how")


def expectation(a, b):
    waits = KIND[a] in WAITS_FOR[KIND[b]]
    return Expect(waits, "data" if KIND[a] == "edit" and KIND[b] == "edit" else "gate")


TABLE = {(a, b): expectation(a, b) for a in OPS for b in OPS}


def case_id(ctx, a, b):
    return "%s:%s->%s" % (ctx, a, b)


def holder_for(b):
    """Edits as A synchronise the caller's stream on the host (device_check), so they cannot sit behind a gate; they are held
    through update_begin instead: Z sits behind the gate on a third stream and the edit waits for Z.  Z is chosen so that B
    has no documented edge to it: a query when B is frame-like (or a filter / accumulate call), a frame when B is a reader."""
    z = "frame" if KIND[b] == "reader" else "query"
    assert not TABLE[(z, b)].waits and TABLE[(z, "update")].waits
    return z


# What each context runs.  A context holds objects or a skin, so pose_skin has a context of its own and a reduced row.
MAIN_OPS = tuple(op for op in OPS if op != "pose_skin")
# An update or a replace drops the object table (rt_update_scene*), so a pose cannot follow one without a blocking
# rt_set_objects in between: those edit -> edit cells do not exist as two-stream sequences.
IMPOSSIBLE = {(a, "pose") for a in ("update", "replace")}


def pairs(rows, columns=MAIN_OPS):
    return [(a, b) for a in rows for b in columns if (a, b) not in IMPOSSIBLE]


CONTEXT_PAIRS = {
    "a": pairs(("frame", "aov", "update", "pose")),                  # the Cornell box: n = 26, the wave kernel
    "b": pairs(MAIN_OPS),                                            # box + 2 346-triangle sphere: the whole matrix
    "c": [("frame", "frame"), ("update", "frame"), ("frame", "update"), ("query", "update"), ("update", "query"),
          ("accumulate", "accumulate")],                             # devices = (0, 0), bands of 8 rows
    "skin": [("pose_skin", b) for b in ("frame", "query", "aov", "filter")] +
            [(a, "pose_skin") for a in ("frame", "query", "aov", "filter")],
}


def all_case_ids():
    return [case_id(ctx, a, b) for ctx in ("a", "b", "c", "skin") for a, b in CONTEXT_PAIRS[ctx]]


# ==== the device part ======================================================================================================
GATE_FACTOR = 50                 # the gate lasts at least this many times the longest operation of the case (A, B, the holder Z)
VOID_FACTOR = 4                  # a void case is run once more with a gate this many times longer
MAX_CANDIDATES = 8


class Clock:
    """torch.cuda._sleep's cycles per millisecond, measured once per session with a pair of events (no clock is assumed).
    Without _sleep the gate is a chain of torch.mm on preallocated 4096^2 tensors, calibrated the same way."""
    _instance = None

    @classmethod
    def get(cls):
        if cls._instance is None:
            cls._instance = cls()
        return cls._instance

    def __init__(self):
        import torch
        self.torch = torch
        self.have_sleep = hasattr(torch.cuda, "_sleep")
        if not self.have_sleep:
            self.mm = [torch.ones((4096, 4096), device="cuda") for _ in range(3)]
        self.units_per_ms = None
        units = 100000 if self.have_sleep else 1
        for _ in range(4):                                   # lengthen the probe until it lasts about 2 ms, then keep that
            ms = self._timed(units)
            if ms >= 2.0:
                break
            units = int(units * max(2.0, 3.0 / max(ms, 1e-3)))
        ms = min(self._timed(units) for _ in range(3))
        self.calibration = (units, ms)
        self.units_per_ms = units / ms

    def _spin(self, units):
        if self.have_sleep:
            self.torch.cuda._sleep(int(units))
        else:
            for _ in range(int(units)):
                self.torch.mm(self.mm[0], self.mm[1], out=self.mm[2])

    def _timed(self, units):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self._spin(units)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def gate(self, stream, ms):
        """A spin of `ms` milliseconds on `stream` and the event right behind it."""
        torch = self.torch
        end = torch.cuda.Event()
        with torch.cuda.stream(stream):
            self._spin(max(1, int(ms * self.units_per_ms)))
            end.record(stream)
        return end

    def describe(self):
        what = "torch.cuda._sleep cycles" if self.have_sleep else "torch.mm 4096^2 products"
        return "calibration: %d %s in %.3f ms -> %.0f per ms" % (self.calibration[0], what, self.calibration[1], self.units_per_ms)


def device_ms(fn, stream):
    """The device time of fn() alone on `stream`, by a pair of events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), host


# ---- the control ----------------------------------------------------------------------------------------------------------
class Control(AssertionError):
    pass


def _completes_while_closed(clock, gated, behind_gate, probes, ms):
    """Gate `gated`, run behind_gate() (may enqueue more on it), then probes: a list of (stream, fn).  -> per probe: did its
    event turn true while the gate's event, read afterwards, was still false?"""
    import torch
    torch.cuda.synchronize()
    end = clock.gate(gated, ms)
    if behind_gate is not None:
        behind_gate()
    events = []
    for stream, fn in probes:
        fn()
        ev = torch.cuda.Event()
        ev.record(stream)
        events.append(ev)
    seen = [False] * len(events)
    while True:
        done = [ev.query() for ev in events]
        closed = not end.query()
        if closed:
            seen = [s or d for s, d in zip(seen, done)]
        if not closed or all(seen):
            break
    torch.cuda.synchronize()
    return seen


def pick_streams(clock, frame_on, frame_as_b=True, report=print):
    """-> (g, e, b): g takes the gate (and A, or the holder Z), e an edit that is held through Z, b takes B.  From at most 8
    torch streams, three such that a trivial operation on each of e and b completes while a gate on g — with a frame of the
    context behind it, which ties up the context's own streams — is closed, and likewise between e and b; with frame_as_b,
    also a frame of the context on b completes while a bare gate on g is closed (the frame's own streams are not g's queue).
    frame_on(stream) enqueues a frame.  Raises Control if there are none: then nothing could be tested."""
    import torch
    cands = [torch.cuda.Stream() for _ in range(MAX_CANDIDATES)]
    cell = torch.zeros(MAX_CANDIDATES, 64, device="cuda")

    def trivial(j):
        def fn():
            with torch.cuda.stream(cands[j]):
                cell[j].add_(1.0)
        return (cands[j], fn)

    # the time of one round of probes alone sizes the probes' gate, like every gate here (the second round: the first one
    # loads code objects)
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(MAX_CANDIDATES):
            trivial(j)[1]()
        frame_on(cands[0])
        torch.cuda.synchronize()
        ms = GATE_FACTOR * (time.perf_counter() - t0) * 1e3
    free = np.zeros((MAX_CANDIDATES, MAX_CANDIDATES), bool)          # free[i, j]: j runs while i is gated with a frame behind
    for i in range(MAX_CANDIDATES):
        others = [j for j in range(MAX_CANDIDATES) if j != i]
        seen = _completes_while_closed(clock, cands[i], lambda: frame_on(cands[i]), [trivial(j) for j in others], ms)
        free[i, others] = seen
    report("control: gate %.2f ms; stream j runs while stream i is gated with a frame behind it (rows i):" % ms)
    for i in range(MAX_CANDIDATES):
        report("  " + " ".join("x" if free[i, j] else "." for j in range(MAX_CANDIDATES)))
    # With frame_as_b: a frame of the context on another queue must complete while g ALONE is gated, or the context's own
    # streams share g's queue and every B that is a frame would be held by the gate itself.  Asked once per hardware queue:
    # two candidates share one if neither runs while the other is gated.
    frame_ok = np.ones(MAX_CANDIDATES, bool)
    for g in range(MAX_CANDIDATES if frame_as_b else 0):
        earlier = [j for j in range(g) if not free[g, j] and not free[j, g]]
        runs_beside = [j for j in range(MAX_CANDIDATES) if free[g, j]]
        if earlier:
            frame_ok[g] = frame_ok[earlier[0]]
        elif runs_beside:
            b = runs_beside[0]
            frame_ok[g] = _completes_while_closed(clock, cands[g], None, [(cands[b], lambda: frame_on(cands[b]))], ms)[0]
        else:
            frame_ok[g] = False
    if frame_as_b:
        report("control: a frame on another queue completes while stream i alone is gated: "
               + " ".join("x" if ok else "." for ok in frame_ok))
    for g, e, b in itertools.permutations(range(MAX_CANDIDATES), 3):
        if frame_ok[g] and free[g, e] and free[g, b] and free[e, b] and free[b, e]:
            report("control: streams g, e, b = candidates %d, %d, %d" % (g, e, b))
            return cands[g], cands[e], cands[b]
    raise Control("control failed: among %d torch streams there are no three on independent hardware queues that are also "
                  "independent of the context's own streams (a trivial operation on one must complete while a gate is "
                  "closed on another) — no ordering case could observe anything, so none was run" % MAX_CANDIDATES)


# ---- one case -------------------------------------------------------------------------------------------------------------
VOID = "void"
LATE = "B had not finished when the gate ahead of A opened: B waits for A (or for something A holds)"


def observe(end, ev_b, waits):
    """After A and B are enqueued and ev_b recorded.  -> None (as expected), VOID, LATE, or what went wrong.  Every reading of
    B's event counts only if the gate's event, read after it, is still unset."""
    if waits:
        # At every look while the gate stays closed, not only at the first one: right after its enqueue B's event is unset
        # whether B waits or not — a B that does not wait still needs its own run time (the gate lasts 50 times that) to finish.
        looks = 0
        while True:
            done = ev_b.query()
            if end.query():
                return None if looks else VOID               # (not one look with the gate closed: nothing was observed)
            if done:
                return "B finished while the gate ahead of A was still closed: B did not wait for A"
            looks += 1
    while True:
        done = ev_b.query()
        if end.query():
            return VOID if done else LATE
        if done:
            return None


def run_once(world, a, b, scale):
    """One run of the case on a freshly reset world.  -> (None | VOID | message, notes)."""
    import torch
    exp = TABLE[(a, b)]
    g, e, s_b = world.streams
    world.reset(a, b)
    if exp.how == "data":                                   # edit -> edit: no gate can hold the first without the second
        world.enqueue(a, 0, e)
        world.enqueue(b, 1, s_b)
        torch.cuda.synchronize()
        return None, ""
    ev_b = torch.cuda.Event()
    edit_a = KIND[a] == "edit"
    z = holder_for(b) if edit_a else None
    ms = world.gate_ms(a, b, z) * scale
    end = world.clock.gate(g, ms)
    if edit_a:
        world.enqueue(z, 0, g)
        closed_a = True                                     # (an edit reads its check back: no such claim for A)
        world.enqueue(a, 0, e)
    else:
        world.enqueue(a, 0, g)
        closed_a = not end.query()
    world.enqueue(b, 1, s_b)
    ev_b.record(s_b)
    closed_b = not end.query()
    result = observe(end, ev_b, exp.waits)
    torch.cuda.synchronize()
    if not (closed_a and closed_b) and result in (None, VOID):
        # the gate was open when an enqueue returned: either the gate was too short (void) or the entry made a host round trip,
        # which a four times longer gate tells apart
        result = VOID
        world.last_void = "the gate had opened when the enqueue of %s returned" % (a if not closed_a else b)
    elif result == VOID:
        world.last_void = "the gate had opened when B's event was read"
    return result, "gate %.2f ms%s" % (ms, ", held through a %s" % z if z else "")


def run_case(world, a, b, report=print):
    """The case (A, B) of DESIGN 4.9 in `world`: observation (void -> once more with a gate four times longer; void again is a
    failure), then the data."""
    result, notes = run_once(world, a, b, 1)
    first = result
    if result == LATE:
        # A B that really waits never finishes behind a closed gate, however long the gate; one that was only slowed down (the
        # device is shared) does.  So a second look with the longer gate cannot hide a wait.
        report("%s -> %s: %s (%s), once more" % (a, b, LATE, notes))
        result, notes = run_once(world, a, b, VOID_FACTOR)
    elif result == VOID:
        report("%s -> %s: void (%s; %s), once more" % (a, b, world.last_void, notes))
        result, notes = run_once(world, a, b, VOID_FACTOR)
    if result == VOID and first is not None:
        result = ("void again with %s: %s — a host round trip in an enqueue (the host waited for the gate), or a gate that is "
                  "too short" % (notes, world.last_void))
    report("%s -> %s: expected %s (%s), %s" % (a, b, "waits" if TABLE[(a, b)].waits else "does not wait", notes or "data only",
                                              result or "observed"))
    assert result is None, "%s -> %s: %s" % (a, b, result)
    world.check_data(a, b)


# ---- a context with everything a case needs ----------------------------------------------------------------------------------
VIEWS = [(0.0, 0.0, [0.0, 0.0, -3.2], [0.0, -0.5, -0.7]), (0.3, 0.1, [0.3, 0.2, -2.6], [0.2, -0.6, -0.4])]
NRAYS = 4096
PLANE = (37, 100)
FILTER_SETS = ((5, "defaults"), (5, "value_0.25"))           # slot 0 (A), slot 1 (B): different inputs, different counters
ACCUM_SETS = ("defaults", "plane_eps_0")
AOV_NAMES = ("prim", "depth", "position", "normal", "albedo")
# One counter depends on which wave runs first and is left out of every comparison: stage A of a radiance call hands the rays
# that reached a diffuse surface their slots with one returning atomic per wave, so the ORDER of the records — and with it how
# stage B's waves group the points, which the lane-level count of their shadow walks sees — varies from run to run.  (Measured
# behind the gate: 12 552 225 ... 12 552 329 for one call; the other seven counters and every output bit are the same.)
UNORDERED_STATS = {"radiance": ("shadow_triangle_tests",)}
STATS_OF = {"aov": "aov_stats", "query": "trace_stats", "shade": "shade_stats", "radiance": "radiance_stats",
            "filter": "filter_stats", "accumulate": "accumulate_stats"}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(_bits(x).ravel(), _bits(y).ravel()) for x, y in zip(got, want))


def make_rays(seed, aim):
    """4 096 rays from inside the box, a third of them aimed at `aim` (the geometry the edits move)."""
    rng = np.random.default_rng(seed)
    start = rng.uniform(-0.9, 0.9, size=(NRAYS, 3)).astype(np.float32)
    d = rng.normal(size=(NRAYS, 3)).astype(np.float32)
    k = NRAYS // 3
    d[:k] = np.asarray(aim, np.float32) + rng.normal(scale=0.15, size=(k, 3)).astype(np.float32) - start[:k]
    return np.ascontiguousarray(np.concatenate([start, d], axis=1))


class World:
    """One context under test: its old scene, the scenes its edits lead to (one per edit kind and slot), preallocated inputs
    and outputs for slot 0 (A, or the holder Z) and slot 1 (B), the bits of fresh contexts of every scene, and the stats of
    every call made alone."""

    def __init__(self, name, cfg, fresh_cfg, old, edits, skin=None, ranges=None, aim=(0.0, 0.0, 0.0), report=print):
        """edits: {"update": (scene0, scene1), "replace": (...), "pose": (xforms0, xforms1), "pose_skin": (bones0, bones1)}"""
        import torch
        from conftest import focal_for
        from uob_raytracer_amd import abi, runtime as rt
        import filter_util as fu
        import accumulate_util as au
        self.torch, self.rt, self.abi, self.fu, self.au = torch, rt, abi, fu, au
        self.name, self.cfg, self.old, self.skin, self.ranges, self.report = name, cfg, old, skin, ranges, report
        self.clock = Clock.get()
        self.focal = focal_for(fresh_cfg)
        self.last_void = ""
        self.edit_kinds = tuple(edits)
        self.ops = tuple(op for op in OPS if KIND[op] != "edit" or op in edits)
        H, W = fresh_cfg.height, fresh_cfg.width
        dev = "cuda"
        # ---- what the edits lead to
        self.new_scene = {}
        for kind, (x0, x1) in edits.items():
            for slot, x in ((0, x0), (1, x1)):
                if kind == "pose":
                    self.new_scene[(kind, slot)] = old.posed(ranges, x)
                elif kind == "pose_skin":
                    self.new_scene[(kind, slot)] = skin.skinned(x)
                else:
                    self.new_scene[(kind, slot)] = x
        # ---- inputs of the scene's readers: slot 0 and slot 1 differ
        fresh = rt.RayTracer(fresh_cfg, old)
        self.rays = [make_rays(100 + slot, aim) for slot in (0, 1)]
        self.points6 = []
        for slot in (0, 1):                                  # shade at the hit points of the slot's rays (their own start on a miss)
            tri, hit = fresh.query_closest_hit(make_rays(200 + slot, aim))
            p6 = np.where((tri >= 0)[:, None], hit[:, 0:6], make_rays(300 + slot, aim))
            self.points6.append(np.ascontiguousarray(p6, np.float32))
        # ---- what fresh contexts give: the old scene in both slots, every scene an edit leads to in the slots it is asked in
        self.ref = {"old": {(op, slot): self._fresh_bits(fresh, op, slot) for op in FRAME_LIKE + READERS for slot in (0, 1)}}
        fresh.close()
        for key, scene in self.new_scene.items():
            fresh = rt.RayTracer(fresh_cfg, scene)
            want = [("frame", 0)] + ([(op, 1) for op in FRAME_LIKE + READERS] if key[1] == 0 else [])
            self.ref[key] = {k: self._fresh_bits(fresh, *k) for k in want}
            fresh.close()
            for k in want:                                   # the check is sharp: the edit shows in what is compared
                assert not _same(self.ref[key][k], self.ref["old"][k]), "test set-up: %s of scene %s equals the old scene's" % (k, key)
        h, w = PLANE
        for slot in (0, 1):
            self.ref["old"][("filter", slot)] = [fu.reference(h, w, *FILTER_SETS[slot])[0]]
            self.ref["old"][("accumulate", slot)] = list(au.reference(h, w, ACCUM_SETS[slot])[:3])
        # ---- device buffers, all preallocated
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.inp, self.out = {}, {}
        for slot in (0, 1):
            self.out[("frame", slot)] = [torch.zeros((H, W), **i32), torch.zeros((H, W, 4), **f32)]
            self.out[("aov", slot)] = [torch.zeros((H, W) + ((4,) if abi.AOV_PLANES[n][1] == 4 else ()),
                                                   **(i32 if abi.AOV_PLANES[n][2] else f32)) for n in AOV_NAMES]
            self.inp[("query", slot)] = torch.from_numpy(self.rays[slot]).to(dev)
            self.out[("query", slot)] = [torch.zeros(NRAYS, **i32), torch.zeros((NRAYS, 10), **f32)]
            self.inp[("shade", slot)] = torch.from_numpy(self.points6[slot]).to(dev)
            self.out[("shade", slot)] = [torch.zeros(NRAYS, **f32), torch.zeros(NRAYS, **i32)]
            self.inp[("radiance", slot)] = torch.from_numpy(self.rays[slot]).to(dev)
            self.out[("radiance", slot)] = [torch.zeros((NRAYS, 4), **f32), torch.zeros(NRAYS, **i32)]
            self.inp[("filter", slot)] = [torch.from_numpy(x.copy()).to(dev) for x in fu.planes(h, w)]
            self.out[("filter", slot)] = [torch.zeros((h, w), **f32)]
            planes, kw = au.call_args(h, w, ACCUM_SETS[slot])
            self.inp[("accumulate", slot)] = ([torch.from_numpy(x.copy()).to(dev) for x in planes], kw)
            self.out[("accumulate", slot)] = [torch.zeros((h, w, abi.HISTORY_WORDS), **f32), torch.zeros((h, w), **f32),
                                              torch.zeros((h, w), **f32)]
            for kind, x in edits.items():
                if kind in ("pose", "pose_skin"):
                    self.inp[(kind, slot)] = torch.from_numpy(np.ascontiguousarray(x[slot], np.float32)).to(dev)
                else:
                    self.inp[(kind, slot)] = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in x[slot].packed()]
        torch.cuda.synchronize()
        # ---- the context, its streams, a warm-up of every operation, the calls made alone
        self.tr = rt.RayTracer(cfg, old)
        # A multi-device context renders on its children's own streams, one per entry of `devices`.  e and b must lie on two
        # queues that hold neither of them (the first half of the control), which leaves the children the other two of the four
        # hardware queues — g's among them.  So in (c) a frame on b while g alone is gated is held by queue sharing, the second
        # half of the control cannot be met, and (c) runs no case that expects a frame as B not to wait: c:frame->frame and
        # c:update->frame are serialised by the children's streams whatever the library does, and it is their data that pins
        # wait_scene and the bands there.
        multi = cfg.num_devices > 1
        assert not multi or not [p for p in CONTEXT_PAIRS[name] if p[1] == "frame" and not TABLE[p].waits]
        self.streams = pick_streams(self.clock, lambda s: self.enqueue("frame", 0, s), frame_as_b=not multi, report=report)
        g = self.streams[0]
        self.alone_stats, self.times = {}, {}
        for round_ in range(2):                              # the first round creates events, counters, scratch; the second is timed
            for op in self.ops:
                for slot in (0, 1):
                    self.reset(op, op)
                    dev_ms, host_ms = device_ms(lambda: self.enqueue(op, slot, g), g)
                    self.times[(op, slot)] = (dev_ms, host_ms)
                    if op in STATS_OF:
                        self.alone_stats[(op, slot)] = getattr(self.tr, STATS_OF[op])()
                    if KIND[op] != "edit":
                        assert _same(self.outputs(op, slot), self.ref["old"][(op, slot)]), \
                            "%s (slot %d) alone differs from a fresh context / the restatement" % (op, slot)
        self.dev_ms = {op: max(self.times[(op, s)][0] for s in (0, 1)) for op in self.ops}
        self.host_ms = {op: max(self.times[(op, s)][1] for s in (0, 1)) for op in self.ops}
        report(self.clock.describe())
        report("context %s: device ms / host enqueue ms of each operation alone" % name)
        for op in self.ops:
            report("  %-10s %8.3f / %6.3f" % (op, self.dev_ms[op], self.host_ms[op]))
        gates = [self.gate_ms(a, b, holder_for(b) if KIND[a] == "edit" and KIND[b] != "edit" else None)
                 for a in self.ops for b in self.ops]
        report("context %s: gate = %d x the longest of A, B and the holder + their host enqueue times: %.2f ... %.2f ms"
               % (name, GATE_FACTOR, min(gates), max(gates)))

    def gate_ms(self, a, b, z=None):
        """From the measurement of the warm-up: 50 x the longest operation of the case, plus the host time of its enqueues."""
        ops = [op for op in (a, b, z) if op is not None]
        return GATE_FACTOR * max(self.dev_ms[op] for op in ops) + sum(self.host_ms[op] for op in ops)

    # -- fresh contexts, through the blocking entries
    def _fresh_bits(self, fresh, op, slot):
        yaw, pitch, cam, light = VIEWS[slot]
        rot = self.rt.rotation_matrix(yaw, pitch)
        if op == "frame":
            return [x.copy() for x in fresh.render(rot, cam, light, self.focal, want_rgb=True)]
        if op == "aov":
            planes = fresh.render_aov(rot, cam, self.focal, sample=0, planes=AOV_NAMES)
            return [planes[n] for n in AOV_NAMES]
        if op == "query":
            return list(fresh.query_closest_hit(self.rays[slot]))
        if op == "shade":
            p6 = self.points6[slot]
            return list(fresh.shade_points(p6[:, 0:3], p6[:, 3:6], light, want_counts=True))
        if op == "radiance":
            return list(fresh.radiance_rays(self.rays[slot], light, want_prim=True))
        raise KeyError(op)

    # -- the device entries
    def enqueue(self, op, slot, stream):
        tr, raw = self.tr, stream.cuda_stream
        yaw, pitch, cam, light = VIEWS[slot]
        rot = self.rt.rotation_matrix(yaw, pitch)
        out = self.out.get((op, slot))
        x = self.inp.get((op, slot))
        if op == "frame":
            tr.render_device(rot, cam, light, self.focal, out[0].data_ptr(), out[1].data_ptr(), stream=raw)
        elif op == "aov":
            tr.render_aov_device(rot, cam, self.focal, sample=0, out=dict(zip(AOV_NAMES, out)), stream=stream)
        elif op == "query":
            tr.query_device(self.abi.RT_TRACE_CLOSEST_HIT, x, out_tri=out[0], out10=out[1], stream=stream)
        elif op == "shade":
            tr.shade_points_device(x, light, out_light=out[0], out_counts=out[1], stream=stream)
        elif op == "radiance":
            tr.radiance_rays_device(x, light, out=out[0], out_prim=out[1], stream=stream)
        elif op == "filter":
            params = dict(self.fu.PARAM_SETS[FILTER_SETS[slot][1]], passes=FILTER_SETS[slot][0])
            tr.filter_plane_device(*x, out=out[0], stream=stream, **params)
        elif op == "accumulate":
            planes, kw = x
            tr.accumulate_plane_device(*planes[:3], prim=planes[3], prev=planes[4], next=out[0], out_mean=out[1],
                                       out_variance=out[2], stream=stream, prev_focal=PLANE[1], **kw)
        elif op == "update":
            tr.update_scene_device(*(t.data_ptr() for t in x), len(self.old), stream=raw)
        elif op == "replace":
            tr.replace_scene_device(*x, stream=stream)
        elif op == "pose":
            tr.pose_objects_device(x, stream=stream)
        elif op == "pose_skin":
            tr.pose_skin_device(x, stream=stream)
        else:
            raise KeyError(op)

    def outputs(self, op, slot):
        self.torch.cuda.synchronize()
        return [t.cpu().numpy() for t in self.out[(op, slot)]]

    def reset(self, a, b):
        """The old scene with rt_init's own tiles, the table a pose of the case needs, cleared outputs; nothing in flight."""
        tr = self.tr
        tr.replace_scene(self.old)                           # blocking; drops the object table and the skin
        if "pose" in (a, b):
            tr.set_objects(self.ranges)
        if "pose_skin" in (a, b):
            self.skin.set(tr)
        for outs in self.out.values():
            for t in outs:
                t.zero_()
        self.torch.cuda.synchronize()

    def frame_now(self):
        yaw, pitch, cam, light = VIEWS[0]
        return [x.copy() for x in self.tr.render(self.rt.rotation_matrix(yaw, pitch), cam, light, self.focal, want_rgb=True)]

    def _stats_match(self, op, slot):
        got, want = dict(getattr(self.tr, STATS_OF[op])()), dict(self.alone_stats[(op, slot)])
        for key in UNORDERED_STATS.get(op, ()):
            got.pop(key), want.pop(key)
        assert got == want, "%s: the stats export reports %r, the call made alone %r" % (op, got, want)

    def check_data(self, a, b):
        """A missing wait would have run B wholly before A: the data pins the same edge from the other side."""
        edit_a, edit_b = KIND[a] == "edit", KIND[b] == "edit"
        if edit_a and edit_b:
            assert _same(self.frame_now(), self.ref[(b, 1)][("frame", 0)]), "the final scene is not the second edit's"
            return
        if edit_a:
            z = holder_for(b)
            assert _same(self.outputs(z, 0), self.ref["old"][(z, 0)]), "the %s that held the edit does not show the old scene" % z
            want = self.ref[(a, 0)][(b, 1)] if KIND[b] in ("frame_like", "reader") else self.ref["old"][(b, 1)]
            assert _same(self.outputs(b, 1), want), "B (%s) does not have the bits of a fresh context of the new scene" % b
            assert _same(self.frame_now(), self.ref[(a, 0)][("frame", 0)]), "a frame after the edit does not show the new scene"
            return
        assert _same(self.outputs(a, 0), self.ref["old"][(a, 0)]), "A (%s) does not have the bits of the old scene / of the call alone" % a
        if edit_b:
            assert _same(self.frame_now(), self.ref[(b, 1)][("frame", 0)]), "a frame right after does not show the new scene"
            return
        assert _same(self.outputs(b, 1), self.ref["old"][(b, 1)]), "B (%s) does not have the bits of the call made alone" % b
        if b in STATS_OF:
            self._stats_match(b, 1)                          # the family's export reports B's counters
        if a in STATS_OF and a != b:
            self._stats_match(a, 0)
        if b in ("filter", "accumulate"):                    # and they are the restatement's
            ref = (self.fu.reference(*PLANE, *FILTER_SETS[1])[1] if b == "filter" else self.au.reference(*PLANE, ACCUM_SETS[1])[3])
            got = getattr(self.tr, STATS_OF[b])()
            assert {k: got[k] for k in ref} == ref

    def close(self):
        self.torch.cuda.synchronize()
        self.tr.close()
