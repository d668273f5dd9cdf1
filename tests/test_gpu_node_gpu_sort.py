"""-m gpu: the Viewer's own runSplatSort text with `gpuAcceleratedSort: true` through the JS drop-ins (tests/gpu_sort_via_viewer.mjs):
SplatMesh.computeDistancesOnGPU fills the worker's precomputed distances with the restated shader (tests/distance_cases.py) over the
shim's own getIntegerCenters / getFloatCenters, and the list handed to updateRenderIndexes is the C oracle's sort of those
distances - for integer and float distances, through the worker's SharedArrayBuffer and through plain typed arrays, with and
without an octree whose gather culls leaves (the index list then names original indexes beyond splatRenderCount)."""
import json
import os
import shutil

import numpy as np
import pytest

import oracle
from distance_cases import shader_distances
from gaussiansplats3d_amd import camera, util
from test_node_seam import ROOT, _bundle, _node, _scene_ply

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def _wide_scene_ply(n, seed):
    """An INRIA-v1 .ply whose splats surround the garden camera (many behind it and beside the frustum): an octree gather for
    that camera keeps only some of the leaves, so splatRenderCount < n and indexesToSort names original indexes up to n - 1."""
    from gaussiansplats3d_amd import assets
    rng = np.random.default_rng(seed)
    pos = np.array(camera.DEMO_POSES["garden"][1])
    centers = (pos + rng.normal(size=(n, 3)) * 6.0).astype(np.float32)
    return assets.write_ply(centers, rng.normal(np.log(0.05), 0.7, size=(n, 3)).astype(np.float32), rng.normal(size=(n, 4)).astype(np.float32),
                            rng.normal(0, 1.0, size=(n, 3)).astype(np.float32), rng.normal(1.0, 2.5, size=n).astype(np.float32), None)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "float"])
@pytest.mark.parametrize("shared,final_build", [(True, False), (False, False), (True, True), (False, True)],
                         ids=["shared", "copied", "shared-tree", "copied-tree"])
def test_gpu_accelerated_sort_through_the_viewer_text(tmp_path, integer, shared, final_build):
    bundle = _bundle()
    n, W, H = 20000, 640, 360
    ply = _wide_scene_ply(n, seed=606) if final_build else _scene_ply(n, 0, seed=505)
    (tmp_path / "scene.ply").write_bytes(ply)
    cam = camera.demo_camera("garden", W, H)
    cfg = dict(width=W, height=H, shDegree=0, fov=camera.THREE_FOV_DEG, matrixWorld=np.asarray(cam.matrix_world).tolist(),
               projection=np.asarray(cam.projection).tolist(), finalBuild=final_build, sharedMemoryForWorkers=shared,
               integer=integer, sceneOptions={})
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    _node([os.path.join(ROOT, "tests", "gpu_sort_via_viewer.mjs"), bundle, str(tmp_path / "scene.ply"), str(tmp_path),
           str(tmp_path / "cfg.json")], timeout=300)
    meta = json.load(open(tmp_path / "meta.json"))
    assert meta["splatCount"] == n and meta["usePrecomputedDistances"] is True and meta["centersPosted"] is False
    dt = np.int32 if integer else np.float32
    centers4 = np.fromfile(tmp_path / "centers.bin", dtype=dt).reshape(n, 4)   # the shim's getIntegerCenters / getFloatCenters
    received = np.fromfile(tmp_path / "distances.bin", dtype=dt)
    handed = np.fromfile(tmp_path / "sorted.u32", dtype=np.uint32)
    listed = np.fromfile(tmp_path / "indexes.u32", dtype=np.uint32)              # that sort's indexesToSort
    mvp = np.asarray(meta["modelViewProj"], np.float64)
    uniforms, _ = util.distance_uniforms(mvp, integer, False)
    want = shader_distances(centers4, uniforms, integer, False)
    assert np.array_equal(received.view(np.uint32), want.view(np.uint32))
    R = meta["splatRenderCount"]
    assert meta["renderCountHanded"] == R == handed.size == listed.size
    if final_build:                                         # the octree gather culled leaves: the list is not 0 .. R - 1
        assert meta["leaves"] > 0 and 0 < R < n and int(listed.max()) >= R
    else:
        assert R == n
    expect = oracle.sort_indexes(listed, centers4, mvp.astype(np.float32), sort_count=meta["lastSortCount"], render_count=R,
                                 use_int=integer, precomputed=want)
    np.testing.assert_array_equal(handed, expect)
    assert np.array_equal(np.sort(handed), np.sort(listed))   # every listed splat drawn once
