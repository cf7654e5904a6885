"""-m gpu: DESIGN.md 4.9 ("Ordering: who waits for whom"), cell by cell, behind a gate.

Every other two-stream test of the suite enqueues A on one stream and B on another with nothing holding A back; at test sizes
A has finished before B's first kernel starts, so deleting a wait leaves them green.  Here a spin kernel of measured length
(ordering_util.Clock.gate) sits ahead of A, so A cannot finish while it spins, and each case observes one cell of the table:

  * "B waits for A": B's event stays unset at every look for as long as the gate's event, read afterwards, is unset too
    (the gate lasts 50 times B's own run time, so a B that did not wait would have finished long before);
  * "B does not wait for A": B's event turns set while the gate's event, read afterwards, is still unset;
  * no host round trip: the enqueues of A (unless it is an edit) and of B returned while the gate was closed;
  * the data: what a missing wait would have spoilt has the bits of a fresh context of the right scene, or of the call made
    alone, and the family's stats export reports B's counters.

An observation made after the gate had opened is void: the case runs once more with a gate four times longer, and a second
void fails.  Edits as A read their check back on the host, so they are held through update_begin by a holder Z behind the gate
(ordering_util.holder_for); edit -> edit is the one cell no gate reaches and is checked by its data only.  Before any case
the control (ordering_util.pick_streams) finds three streams that really run independently of each other and of the
context's own streams; without them the module fails — it neither passes nor skips.  No environment variable is set here.

Case ids are "<context>:<A>-><B>"; contexts: a = the Cornell box, b = box + 2 346-triangle sphere (mesh kernel, HBM records,
tile masks, aux stream), c = devices (0, 0) in bands of 8 rows, skin = box + 140-triangle sphere skinned to two bones."""
import numpy as np
import pytest

import ordering_util as ou
import test_gpu_scene_pose as sp
import test_gpu_scene_skin as sk
import test_gpu_scene_update as su
from uob_raytracer_amd import abi

pytestmark = pytest.mark.gpu

KW = dict(width=64, height=48, aa_x=1, aa_y=1, shadow_samples=2)
xform, rot_y, centre_of = sp.xform, sp.rot_y, sp.centre_of

def _report(line):
    """The calibration, the control's choice, the per-operation times, the gate lengths and each observation (pytest -s)."""
    print(line)


def _box_world(name, cfg, box):
    short, tall = list(range(*np.cumsum(sp.SHORT_BLOCK))), list(range(*np.cumsum(sp.TALL_BLOCK)))
    cs, ct = centre_of(box, *sp.SHORT_BLOCK), centre_of(box, *sp.TALL_BLOCK)
    edits = {
        "update": (box.transformed(short, np.eye(3), (0.25, 0.0, -0.125)), box.transformed(short, np.eye(3), (-0.1, 0.0, -0.2))),
        "replace": (box.transformed(tall, np.eye(3), (0.1, 0.0, -0.2)), box.transformed(tall, np.eye(3), (-0.15, 0.0, -0.1))),
        "pose": (np.stack([xform(rot_y(0.3), (0.1, 0.0, -0.05), about=cs), xform(rot_y(-0.3), (-0.05, 0.0, 0.1), about=ct)]),
                 np.stack([xform(np.diag([-1.0, 1.0, 1.0]), (0.1, 0.0, -0.1), about=cs), xform(rot_y(0.7), about=ct)])),
    }
    return ou.World(name, cfg, abi.make_config(**KW), box, edits, ranges=[sp.SHORT_BLOCK, sp.TALL_BLOCK], aim=0.5 * (cs + ct),
                    report=_report)


def _mesh_world(box, tmp):
    both, nf = su._mesh_scene(box, tmp, 40, 30)
    assert len(both) > 16 * 64                                # tile masks, HBM records
    mesh, cm = slice(26, 26 + nf), centre_of(both, 26, nf)
    move = lambda off: both.transformed(mesh, np.eye(3), off)
    edits = {
        "update": (move((0.2, -0.05, -0.1)), move((-0.2, 0.05, 0.0))),
        "replace": (move((0.0, -0.2, 0.2)), move((0.1, 0.1, -0.2))),
        "pose": (np.stack([xform(rot_y(0.4), (0.1, -0.05, -0.1), about=cm)]), np.stack([xform(rot_y(-0.8), (0.0, 0.0, -0.2), about=cm)])),
    }
    cfg = abi.make_config(**KW)
    return ou.World("b", cfg, cfg, both, edits, ranges=[(26, nf)], aim=cm, report=_report)


def _skin_world(box, tmp):
    both, nf = su._mesh_scene(box, tmp, 10, 8)
    skin, cm = sk.Skin(both, 26, nf, *sk.by_height(both, 26, nf), 2), centre_of(both, 26, nf)
    # (a sphere turned about its own axis looks the same: the upper bone also moves it)
    edits = {"pose_skin": (np.stack([sp.IDENT, xform(rot_y(0.5), (0.15, -0.1, -0.1), about=cm)]),
                           np.stack([sp.IDENT, xform(rot_y(-0.8), (-0.1, 0.05, -0.2), about=cm)]))}
    cfg = abi.make_config(**KW)
    return ou.World("skin", cfg, cfg, both, edits, skin=skin, aim=cm, report=_report)


_current = {"name": None, "world": None, "error": None}


def _close_current():
    if _current["world"] is not None:
        _current["world"].close()
    _current.update(name=None, world=None, error=None)


@pytest.fixture(scope="module")
def worlds(scene, tmp_path_factory):
    """One context at a time (its streams would only crowd the hardware queues of the next): asked for another name, the
    current one is closed.  A context whose set-up failed — the control, above all — fails every case of it with the same
    message, at once."""
    tmp = tmp_path_factory.mktemp("ordering")

    def get(name):
        if _current["name"] != name:
            _close_current()
            _current["name"] = name
            try:
                if name == "a":
                    _current["world"] = _box_world("a", abi.make_config(**KW), scene)
                elif name == "b":
                    _current["world"] = _mesh_world(scene, tmp)
                elif name == "c":
                    _current["world"] = _box_world("c", abi.make_config(devices=(0, 0), device_band_rows=8, **KW), scene)
                else:
                    _current["world"] = _skin_world(scene, tmp)
            except Exception as e:                            # kept and raised again for every case of the context
                _current["error"] = e
        if _current["error"] is not None:
            raise _current["error"]
        return _current["world"]

    yield get
    _close_current()


CASES = [(ctx, a, b) for ctx in ("a", "b", "c", "skin") for a, b in ou.CONTEXT_PAIRS[ctx]]


@pytest.mark.parametrize("ctx,a,b", CASES, ids=[ou.case_id(*c) for c in CASES])
def test_cell(ctx, a, b, worlds):
    ou.run_case(worlds(ctx), a, b, report=_report)
