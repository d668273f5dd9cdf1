"""-m gpu: a real draw tied to the pure function of its host policy (csrc/draw_plan.cpp) and to that function's host model
(draw_plan_ref.py).

What a draw decided - whether the schedule job ran, the shift it read the statistics with, the deep pass and its thresholds, whether
the blend took the order, where the vertex stage ran its block test, the size of the list bins - is read back after every
synchronous draw and must equal the pure function (gs_debug_draw_plan) AND the model, both fed this and the previous camera, the
centre sums of the uploaded scene, and the candidates, share, visible splats and tiles the draw before reported.  The model refuses
an input that fp32 and fp64 could decide differently (a turn of 1.5 bins moves a centre of mass in the middle of the frame by
1.4997 bins: a rounding tie); such a draw is held to the pure function alone and listed in the output."""
import os

import numpy as np
import pytest

import draw_plan_cases as dc
import draw_plan_ref as ref
from gaussiansplats3d_amd import Context, camera
from test_draw_plan import library
from test_gpu_blend_schedule import TURNS, Rig, _turn
from test_gpu_deep import _pile

pytestmark = pytest.mark.gpu

W, H = 320, 200                                            # 70 bins: the smallest frame on which the suite grows deep bins


def _orbit(rig, degrees):
    """The rig's camera carried about its look-at point (axis: up) by this angle from the still pose."""
    a, u = np.radians(degrees), rig.up / np.linalg.norm(rig.up)
    v = rig.pos - rig.look
    pos = rig.look + v * np.cos(a) + np.cross(u, v) * np.sin(a) + u * np.dot(u, v) * (1.0 - np.cos(a))
    return camera.PerspectiveCamera(rig.W, rig.H, tuple(pos), tuple(rig.look), tuple(rig.up))


POLICY_ENV = ("GSPLAT_NO_BLEND_ORDER", "GSPLAT_ORDER_MOTION", "GSPLAT_NO_STAT_SHIFT", "GSPLAT_BLEND_ORDER_STALE",
              "GSPLAT_DEEP_ROW_MAJOR_ON_MOTION", "GSPLAT_DEEP_MIN", "GSPLAT_DEEP_FACTOR", "GSPLAT_NO_BLOCK_CULL", "GSPLAT_NO_BLOCK_LIST",
              "GSPLAT_BLOCK_TEST_ALWAYS", "GSPLAT_NO_DEEP")


def _switches():
    """The draw path's switches as the library reads them from the environment (none is set in a plain run of the suite)."""
    e = os.environ
    return dict(no_blend_order=int("GSPLAT_NO_BLEND_ORDER" in e), order_motion=float(e.get("GSPLAT_ORDER_MOTION", 0.045)),
                no_stat_shift=int("GSPLAT_NO_STAT_SHIFT" in e), blend_order_stale=int("GSPLAT_BLEND_ORDER_STALE" in e),
                deep_row_major_on_motion=int("GSPLAT_DEEP_ROW_MAJOR_ON_MOTION" in e), deep_min=int(e.get("GSPLAT_DEEP_MIN", 4096)),
                deep_factor=int(e.get("GSPLAT_DEEP_FACTOR", 3)), block_cull=int("GSPLAT_NO_BLOCK_CULL" not in e),
                no_block_list=int("GSPLAT_NO_BLOCK_LIST" in e), block_test_always=int("GSPLAT_BLOCK_TEST_ALWAYS" in e))


def test_every_draw_decides_as_the_pure_function_and_the_model(monkeypatch):
    monkeypatch.delenv("GSPLAT_LIST_SHIFT", raising=False)     # (read when a mesh is created: the list bins follow the statistics)
    ctx = Context(0)
    scene = _pile(60000, 41)
    rig = Rig(ctx, scene, W, H)
    centres = scene.centers.astype(np.float64)
    centres = centres[np.isfinite(centres).all(axis=1)]
    sw = _switches()
    no_deep = int("GSPLAT_NO_DEEP" in os.environ)
    path = [rig.cam0] * 4 + [_turn(rig, yaw, pitch) for yaw, pitch in TURNS] + [_orbit(rig, 1.0), _orbit(rig, 13.0)]
    # (+ two draws the deep pass is switched off for: on this scene it keeps the order under any motion, so a REFUSED order - the
    # statistics are of these bins, the view is too far - only shows without it)
    path += [(_orbit(rig, 25.0), "no deep"), (_orbit(rig, 37.0), "no deep")]
    prev_cam, prev = None, None                            # the draw before: its camera and what it reported
    serial, shift, rows, refused = 0, 3, [], []
    for step in path:
        cam, tag = step if isinstance(step, tuple) else (step, "")
        if tag == "no deep":
            rig.mesh.set_deep_pass(False)
            no_deep = 1
        rig.draw(cam)
        sched, share, stats = rig.mesh.blend_schedule(), rig.mesh.view_share(), rig.mesh.last_stats()
        assert not stats.overflowed                        # (a redraw would count as a draw of its own)
        words = [0] * dc.MIRROR_WORDS if prev is None else dc.mirror(
            serial=serial, candidates=prev["candidates"], share=prev["share"], visible=prev["visible"], tiles16=prev["tiles16"])
        inputs = dc.make_inputs(
            was=prev_cam or cam, now=cam, centre_sum=[float(s) for s in centres.sum(axis=0)], centre_n=len(centres), mirror=words,
            stats_valid=int(prev is not None), stats_bins=0 if prev is None else sched["blend_bins"], stats_count=scene.count,
            count=scene.count,
            stats_list_shift=prev["list_shift"] if prev else 0, list_shift=shift, draw_serial=serial, no_deep=no_deep,
            list_current=shift, tiles16=int(stats.tiles16), visible=int(stats.visible_splats),
            measured_visible=prev["visible"] if prev else 0, measured_count=scene.count if prev else 0, **sw)
        got = {"order_wg": int(sched["ran"]), "sx": sched["sx"], "sy": sched["sy"], "deep_pass": int(sched["deep"]),
               "deep_min": sched["deep_min"], "deep_factor": sched["deep_factor"], "order_taken": int(sched["order_taken"]),
               "blend_bins": sched["blend_bins"], "block_test": share["block_test"]}
        pure = library(inputs)
        row = dict(got, list_bin_px=int(stats.list_bin_px), candidates=sched["candidates"], share=sched["share"], tag=tag)
        print(f"draw {serial}: {row}")
        assert int(stats.list_bin_px) == 16 << shift, (serial, stats.list_bin_px, shift)
        assert got == {k: pure[k] for k in got}, (serial, got, {k: pure[k] for k in got})
        try:                                               # (not the unit placement: nothing reads it back from a draw)
            want = ref.plan_schedule(inputs)
            want["list_shift"] = ref.adapt_list_shift(shift, int(stats.tiles16), int(stats.visible_splats))
            want["block_test"] = ref.block_test_mode(inputs["measured_visible"], inputs["measured_count"], 0, sw["block_cull"],
                                                     sw["no_block_list"], sw["block_test_always"])
        except AssertionError as why:                      # a tie fp32 and fp64 could decide differently: the pure function alone
            refused.append((serial, str(why)))
        else:
            assert got == {k: want[k] for k in got}, (serial, got, {k: want[k] for k in got})
            assert {k: pure[k] for k in want} == want, (serial, {k: (pure[k], want[k]) for k in want if pure[k] != want[k]})
        rows.append(dict(row, order_ok=pure["order_ok"]))
        # what the next draw goes by
        prev_cam = cam
        prev = {"candidates": sched["candidates"], "share": sched["share"], "visible": int(stats.visible_splats),
                "tiles16": int(stats.tiles16), "list_shift": shift}
        shift = pure["list_shift"]                         # (the statistics read above re-evaluated the size of the list bins)
        serial += 1
    print(f"{len(refused)} of {len(path)} draws refused by the model (held to the pure function alone): {refused}")
    if not any(k in os.environ for k in POLICY_ENV):         # (under a switch the path need not produce every outcome)
        assert len(refused) <= len(path) // 2, refused
        assert any(r["order_taken"] for r in rows), "no draw took an order"
        assert any(r["order_ok"] and not r["order_taken"] for r in rows), "no draw refused an order it had statistics for"
        assert any(r["sx"] > 0 for r in rows) and any(r["sx"] < 0 for r in rows), "the shift in x took one sign only"
        assert any(r["sy"] > 0 for r in rows) and any(r["sy"] < 0 for r in rows), "the shift in y took one sign only"
        assert any(r["deep_pass"] for r in rows), "no draw ran the deep pass"
    rig.close()
    ctx.close()
