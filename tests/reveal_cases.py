"""tests/golden/reveal_kat.json (recorded from the reference by tests/tools/make_reveal_golden.py) and how a state machine is
replayed against it: the largest distance of every build's range comes from the host model of gs_mesh_bounds (bounds_ref)."""
import json
import math
import os

import numpy as np

import bounds_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reveal_kat.json")
_kat = None


def kat():
    global _kat
    if _kat is None:
        _kat = json.load(open(GOLDEN))
    return _kat


def script(name):
    return next(s for s in kat()["scripts"] if s["name"] == name)


def script_names():
    return [s["name"] for s in kat()["scripts"]]


def script_centers(s):
    return np.asarray(kat()["script_scenes"][s["scene"]], np.float32).reshape(-1, 3)


def range_distance(centers, start, end):
    """max_distance_from of a build whose loop visits [start, end): the root of the model's max_dist_sq."""
    return lambda center: math.sqrt(bounds_ref.bounds(centers, center, start, end - start)["max_dist_sq"])


def replay(s, machine):
    """Runs script `s` on `machine` (reveal.VisibleRegion or a variant of it); yields (where, got, expected) at every recorded point."""
    centers = script_centers(s)
    for e, ev in enumerate(s["events"]):
        if ev["op"] == "build":
            if ev["reset"]:
                machine.reset()
            machine.update(ev["update"], [s["sceneCenter"]], ev["finalBuild"], range_distance(centers, ev["from"], ev["to"]))
            yield (f"{s['name']} event {e} build", list(machine.calculated_scene_center) + machine.state(),
                   ev["calculatedSceneCenter"] + ev["state"])
        else:
            want = {smp[0]: smp[2:] for smp in ev["samples"]}
            for k in range(ev["count"]):
                machine.update_fade_distance(ev["mode"])
                if k in want:
                    yield f"{s['name']} event {e} frame {k}", machine.state(), want[k]


def same(got, expected):
    """Doubles compared with ==, flags by truth value."""
    return len(got) == len(expected) and all((bool(g) == bool(x)) if isinstance(x, bool) else (g == x) for g, x in zip(got, expected))
