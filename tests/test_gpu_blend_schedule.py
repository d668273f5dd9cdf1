"""-m gpu: the blend schedule (csrc/tile_bin.hip, blend_schedule_job) held to its host model (blend_schedule_ref.py).

The schedule orders the blend's 32-px bins by what they cost in the previous draw, names the deep pass's members and raises its
trigger.  None of that changes a pixel, so frame tests cannot see it.  Here every draw k + 1 is checked against the statistics
draw k left (gs_mesh_debug_read 4 - the buffer the schedule reads): the order is a permutation whose model keys never decrease,
and on the kernel's own head of the order (the order inside a key bucket is free) the members, the trigger and the members'
share of the walk are exactly the model's.  Cameras: still, and turning in place, where the schedule reads each bin's cost from a
neighbour (StatShift) - the case in which zeroing the members' statistics while they were still being read dropped members."""
import numpy as np
import pytest

import blend_schedule_ref as ref
from gaussiansplats3d_amd import Context, SplatMesh, camera, create_sort_worker, scenes, util
from test_gpu_deep import _pile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def c3s():
    return scenes.make_config_scene("C3S")


def _turn(rig, yaw_bins, pitch_bins):
    """The rig's camera turned about its own position by about this many 32-px bins: yaw about its up vector, pitch about its
    right vector."""
    fwd = rig.look - rig.pos
    fwd /= np.linalg.norm(fwd)
    u = rig.up / np.linalg.norm(rig.up)
    right = np.cross(fwd, u)
    right /= np.linalg.norm(right)
    f = 0.5 * rig.H / np.tan(np.radians(camera.THREE_FOV_DEG) / 2.0)          # focal length in pixels

    def rot(v, axis, bins):
        a = np.arctan(bins * 32.0 / f)
        return v * np.cos(a) + np.cross(axis, v) * np.sin(a) + axis * np.dot(axis, v) * (1.0 - np.cos(a))

    d = rot(rot(fwd, u, yaw_bins), right, pitch_bins)
    return camera.PerspectiveCamera(rig.W, rig.H, tuple(rig.pos), tuple(rig.pos + 4.0 * d), tuple(rig.up))


# (yaw, pitch) per pose, in bins: steps of 1 - 2 bins, both signs on each axis
TURNS = [(0, 0), (1.5, 0), (3, 0), (1.5, 0), (0, 0), (0, 1.5), (0, 3), (0, 1.5), (0, 0), (-1.5, -1.5), (-3, -2.5), (-1.5, -1), (0, 0)]


class Rig:
    def __init__(self, ctx, scene, W, H, distance=1.0):
        """distance: of the camera from the demo's look-at point, relative to the demo pose's."""
        n = scene.count
        up, pos, look = (np.asarray(v, dtype=np.float64) for v in camera.DEMO_POSES["garden"])
        self.up, self.look, self.pos, self.W, self.H = up, look, look + distance * (pos - look), W, H
        self.cam0 = camera.PerspectiveCamera(W, H, tuple(self.pos), tuple(look), tuple(up))
        self.mesh = SplatMesh(ctx, n, scene.sh_degree, scene.cov_half)
        self.mesh.build(scene.centers, scene.cov, scene.rgba, scene.sh if scene.sh_degree else None)
        self.w = create_sort_worker(ctx, n)
        self.w.post_message({"centers": util.integer_centers(scene.centers), "range": {"from": 0, "to": n - 1, "count": n}})
        self.n = n
        self.checked = []                                  # (sx, sy, deep, members, total) of every draw checked

    def draw(self, cam):
        self.mesh.set_camera(cam)
        self.w.sort_on_device(cam.sort_mvp(), self.n)
        self.mesh.use_sorter_result(self.w, self.n)
        self.mesh.render()                                 # synchronous: the statistics below are this draw's

    def draw_and_check(self, cam):
        stats = self.mesh.blend_bin_stats()                # what the next draw's schedule reads
        self.draw(cam)
        got = self.mesh.blend_schedule()
        if not got["ran"]:
            return got
        B = got["blend_bins"]
        bx = (cam.width + 31) // 32
        assert B == stats.shape[0] * stats.shape[1] and B % bx == 0, (B, stats.shape)
        sch = ref.schedule(stats[..., 1], bx, B, got["sx"], got["sy"], got["deep_min"], got["deep_factor"])
        order = got["order"]
        bad = ref.check_order(sch, order)
        assert not bad, f"shift ({got['sx']}, {got['sy']}): {bad}"
        want = ref.head_outcome(sch, order)
        info = self.mesh.deep_pass_info()
        tag = (f"{cam.width}x{cam.height} shift ({got['sx']}, {got['sy']}) deep={got['deep']}: "
               f"total {sch.total}, thr {sch.thr}, trigger {sch.trigger}, {len(want['members'])} members")
        if got["deep"]:
            have = set(int(b) for b in info["bins"])
            assert len(have) == len(info["bins"]), f"{tag}: a bin named twice"
            assert have == want["members"], (f"{tag}: {len(want['members'] - have)} members missing "
                                             f"{sorted(want['members'] - have)[:10]}, {len(have - want['members'])} extra")
        else:
            assert len(info["bins"]) == 0, tag
        assert info["candidates"] == want["candidates"], f"{tag}: candidates {info['candidates']} != {want['candidates']}"
        assert got["candidates"] == want["candidates"], f"{tag}: mirror[4] {got['candidates']} != {want['candidates']}"
        assert got["share"] == want["share"], f"{tag}: mirror[5] {got['share']} != {want['share']}"
        self.checked.append((got["sx"], got["sy"], got["deep"], len(want["members"]), sch.total))
        return got

    def close(self):
        self.w.terminate()
        self.mesh.dispose()


def _still(rig, draws=4):
    for _ in range(draws):
        got = rig.draw_and_check(rig.cam0)
    assert got["ran"] and (got["sx"], got["sy"]) == (0, 0)
    return got


def _turning(rig, turns=TURNS, need_deep=True):
    for yaw, pitch in turns:
        rig.draw_and_check(_turn(rig, yaw, pitch))
    moved = [c for c in rig.checked if (c[0], c[1]) != (0, 0) and (c[2] or not need_deep)]
    # the case is about reading a NEIGHBOUR's statistics: every direction has to have happened, with the deep pass running
    assert any(c[0] > 0 for c in moved) and any(c[0] < 0 for c in moved), rig.checked
    assert any(c[1] > 0 for c in moved) and any(c[1] < 0 for c in moved), rig.checked
    return moved


@pytest.mark.parametrize("W,H", [(320, 200), (640, 480)])      # 70 bins (< 256), 300 bins (256 .. 512)
def test_schedule_matches_the_model_on_the_deep_pile(ctx, W, H):
    rig = Rig(ctx, _pile(60000, 41), W, H)
    rig.draw(rig.cam0)
    got = _still(rig)
    assert got["deep"] and len(rig.mesh.deep_pass_info()["bins"]) >= 1       # the pile does make deep bins
    assert (got["blend_bins"] < 256) == (W == 320) and (256 < got["blend_bins"] <= 512) == (W == 640)
    _turning(rig, need_deep=False)
    rig.close()


def test_schedule_matches_the_model_on_capture_like_1080p_still_and_turning(ctx, c3s):
    # (closer than the demo pose: from there the object's costly bins outnumber the 256 threads of the schedule's workgroup -
    # at the demo pose ~240 bins qualify, and a member zeroed early was then never read again by a later position)
    rig = Rig(ctx, c3s, 1920, 1080, distance=0.6)
    rig.draw(rig.cam0)
    got = _still(rig)
    assert got["blend_bins"] == 2040 and got["deep"]
    moved = _turning(rig)
    # the shifted draws have a costly run of more than 256 head bins: the deep pass's second half of the head is exercised
    assert max(c[3] for c in moved) > 256, rig.checked
    print("C3S 1080p schedule checks (sx, sy, deep, members, total):", rig.checked)
    rig.close()


def test_schedule_without_the_deep_pass(ctx, c3s):
    rig = Rig(ctx, c3s, 1920, 1080)
    rig.mesh.set_deep_pass(False)
    rig.draw(rig.cam0)
    got = _still(rig)
    assert not got["deep"] and got["candidates"] > 0        # the trigger is still raised, nobody is named
    rig.close()


def test_schedule_total_at_the_largest_ordered_frame(ctx, c3s):
    """The schedule orders frames of up to 8192 bins (4K: 120 x 68 = 8160); its cost total is a uint32 sum over them.  The exact
    model's total, scale shift and mirror words are the kernel's there - and an 8K frame (32 400 bins) is not ordered at all."""
    rig = Rig(ctx, c3s, 3840, 2160)
    rig.draw(rig.cam0)
    got = _still(rig, draws=3)
    assert got["blend_bins"] == 8160
    print("C3S 4K schedule total:", max(c[4] for c in rig.checked), "of", 2 ** 32)
    rig.close()
    rig = Rig(ctx, c3s, 7680, 4320)
    for _ in range(3):
        rig.draw(rig.cam0)
    got = rig.mesh.blend_schedule()
    assert not got["ran"] and got["blend_bins"] == 32400 and got["order"] is None
    rig.close()
