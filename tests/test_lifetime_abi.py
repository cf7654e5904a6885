"""CPU: rt_debug_live_device_objects — what the library's owners of device memory, events and streams hold in this process —
is declared with the documented signature, exported and bound; it takes no context and needs no device; a fresh process
reports four zeros, and still four zeros after an rt_init that fails for lack of a device (RT_E_DEVICE): the half-built
context gives back whatever it took."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from conftest import ROOT
from uob_raytracer_amd import abi, runtime as rt

SIGNATURE = r"int rt_debug_live_device_objects\(int64_t \w+\[4\]\);"

# A process of its own, with nothing in it but the library (plain ctypes: no torch, no HIP call before the export's first):
# the counters, then an rt_init of one triangle, then the counters again
FRESH_PROCESS = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from uob_raytracer_amd import abi
L = C.CDLL(sys.argv[2])
L.rt_last_error.restype = C.c_char_p
L.rt_destroy.argtypes = [C.c_void_p]
L.rt_destroy.restype = None
def live():
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    assert L.rt_debug_live_device_objects(out) == abi.RT_OK
    return list(out)
first = live()
cfg = abi.make_config(width=64, height=48, shadow_samples=4)
v = (C.c_float * 12)(0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1)
nr = (C.c_float * 4)(0, 0, -1, 1)
col = (C.c_float * 4)(0.5, 0.5, 0.5, 1)
h = C.c_void_p()
rc = L.rt_init(C.byref(cfg), v, nr, col, 1, C.byref(h))
msg = L.rt_last_error().decode(errors="replace")
after_init = live()
if rc == abi.RT_OK:
    L.rt_destroy(h)
print(json.dumps({"first": first, "rc": rc, "msg": msg, "handle": bool(h.value), "after_init": after_init, "last": live()}))
"""


def test_declared_exported_and_bound():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "uob_rt.h")).read())
    assert re.search(SIGNATURE, src)
    assert hasattr(C.CDLL(rt.LIB_PATH), "rt_debug_live_device_objects")
    assert "rt_debug_live_device_objects" in rt.EXPORTS
    assert rt.lib().rt_debug_live_device_objects.argtypes == [C.POINTER(C.c_int64)]
    assert rt.lib().rt_abi_version() == abi.RT_ABI_VERSION == 2          # an addition only
    assert rt.LIVE_OBJECT_KEYS == ("allocations", "bytes", "events", "streams")
    assert sorted(rt.live_device_objects()) == sorted(rt.LIVE_OBJECT_KEYS)


def test_null_argument_is_invalid():
    assert rt.lib().rt_debug_live_device_objects(None) == abi.RT_E_INVALID
    assert "rt_debug_live_device_objects" in rt.lib().rt_last_error().decode()


def test_fresh_process_holds_nothing_and_a_failed_init_gives_everything_back():
    import torch
    run = subprocess.run([sys.executable, "-c", FRESH_PROCESS, ROOT, rt.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    got = json.loads(run.stdout.strip().splitlines()[-1])
    assert got["first"] == [0, 0, 0, 0]
    if not torch.cuda.is_available():                 # here: no device, so rt_init must fail, loudly, and leave nothing
        assert got["rc"] == abi.RT_E_DEVICE and got["msg"] and not got["handle"]
        assert got["after_init"] == [0, 0, 0, 0]
    else:                                             # with a device the context lives until rt_destroy
        assert got["rc"] == abi.RT_OK
        assert got["after_init"][0] > 0 and got["after_init"][1] > 0 and got["after_init"][2] >= 2 and got["after_init"][3] == 1
    assert got["last"] == [0, 0, 0, 0]
