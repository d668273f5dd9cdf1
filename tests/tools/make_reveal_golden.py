"""tests/tools/make_reveal_golden.py — records tests/golden/reveal_kat.json: what the REFERENCE's own SplatMesh.updateVisibleRegion,
updateVisibleRegionFadeDistance and computeBoundingBox compute for seeded centres.  Runs only where the reference tree and Node
exist: tests/tools/reveal_ref.mjs cuts those methods' text out of src/splatmesh/SplatMesh.js at run time and evaluates it against
a stub whose centres come from the reference's own SplatBuffer.getSplatCenter (imported in place through
tests/tools/formats_loader.mjs).  Only numbers are written.

(a) bounds cases: `identity` (300 centres, one scene), `static` (the same centres under a rotation + non-uniform scale +
    translation), `two_scenes` (150 + 150 centres, two transforms, two scene centres): the averaged scene centre, the largest
    distance as an exact double, computeBoundingBox(false / true), and the Float32Array the transformed fill returns.
(b) scripts over 300 centres laid out in shells around the scene centre, so that a progressive load grows the radius step by step:
    final_default, final_gradual, instant, multiplier_5, progressive (a first build, four update builds - the second grows the radius
    by less than VISIBLE_REGION_EXPANSION_DELTA, the third adds only splats inside it - then the final build), rebuild_reset (a
    non-update rebuild with preserveVisibleRegion = false), and boundary_099 over 41 centres of its own, whose fade-in percentage
    lands on 0.99 exactly.  After every build the whole state; of every run of frames the first 50, every 25th, the last and the
    one at which fadeInComplete flips.
usage: python tests/tools/make_reveal_golden.py [<reference/src>]"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFAULT, GRADUAL, INSTANT = 0, 1, 2
RATE_ONE = 333.3333333333333          # SCENE_FADEIN_RATE_GRADUAL * RATE_ONE == 1.0 in double


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return [*(a * np.sin(angle / 2)).tolist(), float(np.cos(angle / 2))]


IDENTITY = {"position": [0, 0, 0], "quaternion": [0, 0, 0, 1], "scale": [1, 1, 1]}
XF_A = {"position": [1.25, -0.5, 2.0], "quaternion": quat([1, 2, 3], 0.7), "scale": [1.5, 0.75, 2.0]}
XF_B = {"position": [-3.0, 0.25, 0.5], "quaternion": quat([-1, 0.5, 0.2], 2.1), "scale": [0.5, 1.25, 1.0]}


def cloud(n, seed, spread=4.0, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * spread + np.asarray(offset)).astype(np.float32)


def shells(seed, center):
    """300 centres in shells around `center`, by index: [0, 60) within 2, [60, 120) within 2..4, [120, 180) within 3..4.6 (grows
    the radius by < 1), [180, 240) within 1..3 (does not grow it), [240, 280) within 5..9, [280, 300) within 6..11."""
    rng = np.random.default_rng(seed)
    bands = [(60, 0.0, 2.0), (60, 2.0, 4.0), (60, 3.0, 4.6), (60, 1.0, 3.0), (40, 5.0, 9.0), (20, 6.0, 11.0)]
    out = []
    for n, lo, hi in bands:
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = rng.uniform(lo, hi, size=(n, 1))
        r[0] = hi                                             # every band reaches its outer radius
        out.append(d * r + np.asarray(center))
    return np.concatenate(out).astype(np.float32)


def scene(centers, scene_center, xf):
    return {"centers": centers.reshape(-1).astype(np.float64).tolist(), "sceneCenter": list(scene_center), **xf}


def build(count, update, final, reset=False):
    return {"op": "build", "count": count, "update": update, "finalBuild": final, "reset": reset}


def frames(count, mode=DEFAULT):
    return {"op": "frames", "count": count, "mode": mode}


def spec():
    c300 = cloud(300, 11, offset=(0.5, -1.0, 2.0))
    ca, cb = cloud(150, 12, 3.0), cloud(150, 13, 5.0, (2.0, 0.0, -1.0))
    bounds = [{"name": "identity", "scenes": [scene(c300, (0.5, -1.0, 2.0), IDENTITY)]},
              {"name": "static", "scenes": [scene(c300, (0.5, -1.0, 2.0), XF_A)]},
              {"name": "two_scenes", "scenes": [scene(ca, (0.1, 0.2, -0.3), XF_A), scene(cb, (2.0, 0.0, -1.0), XF_B)]}]
    sc = (0.25, -0.75, 1.5)
    sh = scene(shells(21, sc), sc, IDENTITY)
    final = build(300, False, True)
    scripts = [{"name": "final_default", "multiplier": 1.0, "events": [final, frames(450)]},
               {"name": "final_gradual", "multiplier": 1.0, "events": [final, frames(1700, GRADUAL)]},
               {"name": "instant", "multiplier": 1.0, "events": [final, frames(30, INSTANT)]},
               {"name": "multiplier_5", "multiplier": 5.0, "events": [final, frames(120)]},
               {"name": "progressive", "multiplier": 1.0,
                "events": [build(60, False, False), frames(40), build(120, True, False), frames(40), build(180, True, False), frames(40),
                           build(240, True, False), frames(40), build(280, True, False), frames(40), build(300, True, True), frames(450)]},
               {"name": "rebuild_reset", "multiplier": 1.0, "events": [final, frames(100), build(300, False, True, reset=True), frames(450)]}]
    for s in scripts:
        s["scene"], s["sceneName"] = sh, "shells"
    # the comparison `fadeInPercentage > 0.99` AT 0.99: the farthest centre is exactly 100 away, a build that is not final keeps
    # visibleRegionRadius = 100 - 1, and a multiplier that makes the gradual rate exactly 1 puts the fade start radius on 99 at once
    far = np.concatenate([cloud(40, 31, 10.0), np.array([[100.0, 0.0, 0.0]], np.float32)])
    assert 0.003 * RATE_ONE == 1.0 and 99 / 100 == 0.99
    scripts.append({"name": "boundary_099", "multiplier": RATE_ONE, "scene": scene(far, (0.0, 0.0, 0.0), IDENTITY), "sceneName": "far",
                    "events": [build(41, False, False), frames(5), frames(5, GRADUAL)]})
    return {"bounds": bounds, "scripts": scripts}


FIELDS = ["maxSplatDistanceFromSceneCenter", "visibleRegionBufferRadius", "visibleRegionRadius", "visibleRegionFadeStartRadius",
          "visibleRegionChanging", "shaderFadeInComplete"]


def main():
    ref_src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
    assert os.path.isdir(ref_src), "reference not present"
    tools = os.path.join(ROOT, "tests", "tools")
    s = spec()
    with tempfile.TemporaryDirectory() as d:
        json.dump(s, open(os.path.join(d, "spec.json"), "w"))
        subprocess.check_call(["node", "--no-warnings", "--experimental-loader", os.path.join(tools, "formats_loader.mjs"),
                               os.path.join(tools, "reveal_ref.mjs"), ref_src, os.path.join(d, "spec.json"), os.path.join(d, "out.json")],
                              cwd=os.path.join(ROOT, "oracle"), stdout=subprocess.DEVNULL)
        ref = json.load(open(os.path.join(d, "out.json")))
    assert ref["modes"] == {"Default": DEFAULT, "Gradual": GRADUAL, "Instant": INSTANT}, ref["modes"]
    out = {"constants": ref["constants"], "modes": ref["modes"], "fields": FIELDS, "bounds": [], "scripts": []}
    for c, r in zip(s["bounds"], ref["bounds"]):
        r["centers"] = [sc["centers"] for sc in c["scenes"]]                     # fp32 values, per scene
        out["bounds"].append(r)
    pack = lambda st: [st[f] for f in FIELDS]                                    # noqa: E731
    for c, r in zip(s["scripts"], ref["scripts"]):
        flips = 0
        for ev in r["events"]:
            if ev["op"] == "build":
                ev["calculatedSceneCenter"] = ev["state"]["calculatedSceneCenter"]
                ev["state"] = pack(ev["state"])
            else:
                flips += sum(1 for smp in ev["samples"] if smp["flip"])
                ev["samples"] = [[smp["k"], int(smp["flip"])] + pack(smp["state"]) for smp in ev["samples"]]
        r["flips"] = flips
        out["scripts"].append(r)
        r["scene"] = c["sceneName"]
    out["script_scenes"] = {c["sceneName"]: c["scene"]["centers"] for c in s["scripts"]}
    by = {r["name"]: r for r in out["scripts"]}
    assert by["final_default"]["flips"] == 1 and by["final_gradual"]["flips"] == 1 and by["multiplier_5"]["flips"] == 1
    assert by["progressive"]["flips"] >= 1 and by["rebuild_reset"]["flips"] >= 1
    builds = [ev for ev in by["progressive"]["events"] if ev["op"] == "build"]
    grown = [b["state"][1] for b in builds]                                      # visibleRegionBufferRadius after each build
    assert len(builds) == 6 and grown[2] == grown[1] and builds[2]["state"][0] > builds[1]["state"][0], grown   # the < 1 step: no expansion
    assert builds[3]["state"][0] == builds[2]["state"][0] and grown[3] == grown[2]     # a range that lies inside: the maximum is a running one
    assert all(grown[k] > grown[k - 1] for k in (1, 4, 5)), grown
    edge = by["boundary_099"]["events"]
    assert edge[0]["state"][:4] == [100.0, 100.0, 99.0, 99.0] and edge[0]["state"][4] is True and by["boundary_099"]["flips"] == 0
    path = os.path.join(GOLDEN, "reveal_kat.json")
    json.dump(out, open(path, "w"), separators=(",", ":"))
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print({r["name"]: r["flips"] for r in out["scripts"]}, size // 1024, "KiB")


if __name__ == "__main__":
    main()
