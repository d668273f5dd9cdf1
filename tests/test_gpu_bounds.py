"""-m gpu: gs_mesh_bounds against its host model (bounds_ref), bit for bit in all three outputs - the count, the fp32 box and the
fp64 squared distance - over wave, storage-block and upload edges, both storage orders, per-scene transforms, NaN / Inf centres
and the ranges it must refuse; then against what the reference itself computed (tests/golden/reveal_kat.json)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bounds_ref
import reveal_cases
from gaussiansplats3d_amd import Context, GsError, SplatMesh
from gaussiansplats3d_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER = (0.3, -1.7, 2.9)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * 5.0 + rng.normal(size=(1, 3))).astype(np.float32)


def mesh_of(ctx, centers, capacity=None, uploads=None, scene_indexes=None, **kw):
    n = len(centers)
    mesh = SplatMesh(ctx, capacity or n, 0, **kw)
    cov = np.tile(np.array([1e-3, 0, 0, 1e-3, 0, 1e-3], np.float32), (n, 1))
    rgba = np.full((n, 4), 128, np.uint8)
    for a, b in uploads or [(0, n)]:
        mesh.build(centers[a:b], cov[a:b], rgba[a:b], start=a, scene_indexes=None if scene_indexes is None else scene_indexes[a:b])
    return mesh


def same(got, want):
    assert got["count"] == want["count"], (got, want)
    assert got["min"].tobytes() == np.asarray(want["min"], np.float32).tobytes(), (got, want)
    assert got["max"].tobytes() == np.asarray(want["max"], np.float32).tobytes(), (got, want)
    assert np.float64(got["max_dist_sq"]).tobytes() == np.float64(want["max_dist_sq"]).tobytes(), (got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_bounds_match_the_model(ctx, n):
    c = cloud(n, 100 + n)
    mesh = mesh_of(ctx, c)
    same(mesh.bounds(0, n, CENTER), bounds_ref.bounds(c, CENTER))
    lo, hi = mesh.compute_bounding_box()
    assert lo.tobytes() == c.min(axis=0).tobytes() and hi.tobytes() == c.max(axis=0).tobytes()
    mesh.dispose()


@pytest.mark.parametrize("keep_order", [False, True], ids=["morton", "keep_order"])
def test_ranges_of_a_mesh_filled_by_two_uploads(ctx, keep_order):
    c = cloud(1000, 7)
    mesh = mesh_of(ctx, c, uploads=[(0, 300), (300, 1000)], keep_order=keep_order)
    for start, count in [(0, 300), (300, 700), (250, 100), (0, 1000)]:
        same(mesh.bounds(start, count, CENTER), bounds_ref.bounds(c, CENTER, start, count))
    mesh.dispose()


def test_two_scenes_with_their_transforms(ctx):
    k = next(c for c in reveal_cases.kat()["bounds"] if c["name"] == "two_scenes")
    transforms = np.asarray(k["transforms"], np.float64)
    c = cloud(600, 9)
    idx = (np.arange(600) >= 250).astype(np.uint32)
    mesh = mesh_of(ctx, c, uploads=[(0, 400), (400, 600)], scene_indexes=idx, dynamic_mode=True)
    for start, count in [(0, 600), (200, 100), (250, 350)]:
        same(mesh.bounds(start, count, CENTER, transforms), bounds_ref.bounds(c, CENTER, start, count, transforms, idx))
    same(mesh.bounds(0, 600, CENTER), bounds_ref.bounds(c, CENTER))      # no flag: the stored centres
    mesh.set_scenes(transforms=list(transforms))
    lo, hi = mesh.compute_bounding_box(True, 1)
    want = bounds_ref.bounds(c, (0, 0, 0), 250, 350, transforms, idx)
    assert lo.tobytes() == want["min"].tobytes() and hi.tobytes() == want["max"].tobytes()
    with pytest.raises(ValueError, match="Invalid scene index"):
        mesh.compute_bounding_box(False, 2)
    mesh.dispose()


def test_nan_is_skipped_and_inf_propagates(ctx):
    c = cloud(500, 11)
    c[137, 1] = np.nan
    c[300] = np.nan
    mesh = mesh_of(ctx, c)
    got = mesh.bounds(0, 500, CENTER)
    same(got, bounds_ref.bounds(c, CENTER))
    assert got["count"] == 498 and np.isfinite(got["max_dist_sq"])
    mesh.dispose()
    c[41, 2] = np.inf
    mesh = mesh_of(ctx, c)
    got = mesh.bounds(0, 500, CENTER)
    same(got, bounds_ref.bounds(c, CENTER))
    assert got["count"] == 498 and got["max"][2] == np.inf and got["max_dist_sq"] == np.inf
    same(mesh.bounds(300, 1, CENTER), bounds_ref.bounds(c, CENTER, 300, 1))        # nothing but a NaN splat: all zero
    mesh.dispose()


def test_an_empty_range_and_a_range_that_is_not_uploaded(ctx):
    c = cloud(300, 13)
    mesh = mesh_of(ctx, c, capacity=1000)
    got = mesh.bounds(120, 0, CENTER)
    assert got["count"] == 0 and got["max_dist_sq"] == 0.0 and not got["min"].any() and not got["max"].any()
    out = L.Bounds(count=77, max_dist_sq=-3.0)
    center = (L.C.c_double * 3)(*CENTER)
    for start, count in [(0, 301), (299, 2), (300, 1), (900, 50), (0xFFFFFFF0, 0x20)]:
        st = mesh.lib.gs_mesh_bounds(mesh.handle, start, count, L.C.cast(center, L.C.c_void_p), None, 0, 0, L.C.byref(out))
        assert st == L.GS_ERR_INVALID, (start, count, st)
        assert out.count == 77 and out.max_dist_sq == -3.0, "out was written"
    with pytest.raises(GsError):
        mesh.bounds(0, 301, CENTER)
    mesh.build(c[:100], np.zeros((100, 6), np.float32), np.zeros((100, 4), np.uint8), start=600)       # a second, detached range
    same(mesh.bounds(600, 100, CENTER), bounds_ref.bounds(c, CENTER, 0, 100))
    with pytest.raises(GsError):
        mesh.bounds(250, 400, CENTER)                                             # spans the gap between the two
    mesh.dispose()


def _golden(name):
    k = next(c for c in reveal_cases.kat()["bounds"] if c["name"] == name)
    per_scene = [np.asarray(x, np.float32).reshape(-1, 3) for x in k["centers"]]
    idx = np.concatenate([np.full(len(x), s, np.uint32) for s, x in enumerate(per_scene)])
    return k, np.concatenate(per_scene), idx


@pytest.mark.parametrize("name", ["identity", "static", "two_scenes"])
def test_the_reference_values_with_the_transforms_applied_on_the_device(ctx, name):
    """A dynamic mesh stores the floats the reference reads: bit-equal to its updateVisibleRegion and computeBoundingBox."""
    k, c, idx = _golden(name)
    mesh = mesh_of(ctx, c, scene_indexes=idx, dynamic_mode=True)
    mesh.set_scenes(transforms=k["transforms"])
    region = mesh.update_visible_region(False, k["sceneCenters"], final_build=True)
    assert region.calculated_scene_center == k["calculatedSceneCenter"]
    assert region.max_splat_distance_from_scene_center == k["maxSplatDistanceFromSceneCenter"]
    assert region.visible_region_radius == region.visible_region_buffer_radius == k["maxSplatDistanceFromSceneCenter"]
    for apply, box in [(False, k["boxPlain"]), (True, k["boxTransformed"])]:
        lo, hi = mesh.compute_bounding_box(apply)
        assert lo.tolist() == box["min"] and hi.tolist() == box["max"], (apply, lo, hi, box)
    mesh.dispose()


@pytest.mark.parametrize("name", ["identity", "static", "two_scenes"])
def test_the_reference_values_with_the_transforms_baked(ctx, name):
    """A static mesh stores the Float32Array the transformed fill returned: the box is the reference's, the radius within the
    derived 2^-24 (R + |center|) of it - and bit-equal where the transform is the identity."""
    k, c, idx = _golden(name)
    baked = np.asarray(k["bakedCenters"], np.float32).reshape(-1, 3)
    mesh = mesh_of(ctx, baked)
    region = mesh.update_visible_region(False, k["sceneCenters"], final_build=True)
    R, got = k["maxSplatDistanceFromSceneCenter"], region.max_splat_distance_from_scene_center
    print(name, "radius", got, "reference", R, "difference", got - R)
    if name == "identity":
        assert got == R
    assert abs(got - R) <= 2.0 ** -24 * (R + float(np.linalg.norm(k["calculatedSceneCenter"])))
    lo, hi = mesh.compute_bounding_box(True)
    assert lo.tolist() == k["boxTransformed"]["min"] and hi.tolist() == k["boxTransformed"]["max"]
    mesh.dispose()


def test_under_poisoned_allocations_in_a_child_process():
    """Every fresh allocation holds 0xFF (NaN as a float, 4294967295 as an index): a read beyond what was uploaded, or of a
    partial no workgroup wrote, shows."""
    env = dict(os.environ, GSPLAT_POISON_ALLOC="0xFF")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tests", "tools", "bounds_child.py")], env=env, text=True, timeout=120)
    rows = json.loads(out.strip().splitlines()[-1])
    assert len(rows) == 4
    c = cloud(700, 17)
    idx = (np.arange(700) % 2).astype(np.uint32)
    transforms = np.asarray(next(b for b in reveal_cases.kat()["bounds"] if b["name"] == "two_scenes")["transforms"], np.float64)
    for row in rows:
        t = transforms if row["transformed"] else None
        want = bounds_ref.bounds(c, CENTER, row["start"], row["count"], t, idx if row["transformed"] else None)
        got = {"count": row["count_out"], "min": np.array(row["min"], np.float32), "max": np.array(row["max"], np.float32),
               "max_dist_sq": float.fromhex(row["max_dist_sq"])}
        same(got, want)
    assert math.isfinite(float.fromhex(rows[0]["max_dist_sq"]))
