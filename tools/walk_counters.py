"""Records the work counters of the inputs of tests/test_gpu_walk_shapes.py, for that test to compare against: the AOV passes, one closest-hit query,
one in-shadow query and one radiance call of tests/walk_shapes_util.py, run twice; a counter that differs between the
two runs is left out (and named on stderr).  The library is the one runtime.py loads, i.e. UOB_RT_LIB where set (as
tools/ab_time.py): point it at a build of the commit whose counters are to be the record.
usage: walk_counters.py [out.json]     (default: tests/golden/walk_counters.json)"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import walk_shapes_util as ws  # noqa: E402


def record(tmpdir):
    out = {}
    for name in ws.SCENES:
        sc = ws.build_scene(name, tmpdir)
        out[name] = {"aov": {}}
        for pass_name in ws.PASSES:
            tr, planes, stats = ws.run_pass(sc, pass_name)
            out[name]["aov"][pass_name] = stats
            if pass_name == ws.CALLS_PASS:
                out[name].update(ws.run_calls(tr, ws.rays_of_pass(planes))[0])
            tr.close()
    return out


def common(a, b, where):
    """The entries that two recordings agree on"""
    if not isinstance(a, dict):
        return a
    keep = {}
    for k in a:
        if isinstance(a[k], dict) or a[k] == b[k]:
            keep[k] = common(a[k], b[k], where + [k])
        else:
            print("not reproducible, left out:", "/".join(where + [k]), a[k], b[k], file=sys.stderr)
    return keep


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "walk_counters.json")
    with tempfile.TemporaryDirectory() as d:
        first, second = record(d), record(d)
    with open(path, "w") as f:
        json.dump(common(first, second, []), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
