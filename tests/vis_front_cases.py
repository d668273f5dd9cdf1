"""The case list of the visibility-culled sort's front-end tests (test_vis_front_ref.py on the CPU, test_gpu_vis_front.py and
tools/vis_front_child.py on the device): a scene whose visibility mask the test dictates splat by splat, the mask patterns, the
sizes, and the rig that runs one (size, pattern, path) comparison against the sort oracle.

The mask is not injectable, so the scene makes it.  Centres lie in a thin column along the garden camera's view axis (depth 2 to 8,
the centres' lateral sigma 0.05 clipped at 3 sigma, a small isotropic covariance, SH-0): every splat in front of the camera is
drawn.  (The covariance is 9e-4 on the diagonal, a splat sigma of 0.03 - the lateral spread of the centres is not what this is
about: the device's mask holds what the frame DRAWS, and its vertex stage drops a splat whose ellipse covers no pixel centre.  With
the shader's clamp of the eigenvalue discriminant at 0.1, a splat sigma of 0.01 projects to an ellipse a third of a pixel wide at
depth 8, which the raster oracle calls visible and the device rightly does not draw.)  Two switches hide a splat:
  * geometry: a fixed set of runs of original indexes (behind_set) is mirrored to negative depth.  Those splats fail the frustum
    test and fill storage blocks of their own with no survivor at all (block_any gating of the derived mask);
  * scene visibility: the mesh is built with enable_optional_effects, per-splat scene indexes are 0 or 1 and set_scenes(visible=
    [1, 0]) hides scene 1.  Hidden and kept splats share storage blocks; a new pattern is one upload of scene indexes, and
    visible=[0, 1] is the complement among the splats in front with no upload at all.
So for a pattern P (bool per splat) the expected mask is  want = P & ~behind,  and the sort oracle runs once per size.  (The
behind set is fixed per size - moving a centre changes the sort keys - so "all" means every splat in front, and the share of the
hidden splats that is hidden by geometry varies with the pattern: about a ninth of the positions lie behind.)"""
import numpy as np

import vis_front_ref as ref

W, H = 160, 128                       # 8 tile rows; the column projects to the centre of the frame
STRIP, FAR_STRIP = (3, 5), (0, 1)     # the centre tile rows (pixel rows 48 .. 80) / rows the column never reaches
SHORT = (37, 38)                      # lists shorter than the projection by these many positions (R % 4 == 0 and == 3 for n % 4 == 1)
NONCOARSE = 16_777_217                # 65537 storage blocks: k_mask_derive_count's non-coarse branch
FRAME_ALWAYS = 1_200_000              # splats up to which every comparison also draws the unculled sort's frame (Rig.run)
SMALL = (1, 3, 31, 32, 33, 63, 64, 65)
SMALL_PATTERNS = ("all", "none", "first", "last", "rand30", "mod5")


def sizes(T):
    """{label: R} for T = 2 x CUs workgroups.  A turn of k_cull_front is VC_TURN = 2048 positions: T*2048 is the last size with one
    turn per workgroup of the streaming front end, T*2048 + 1 the first with two (half the workgroups own 4096 positions, one owns a
    single position, the rest are empty), T*4096 + 1 the first with three (s_turn reused); T*1024 + 1 is k_minmax_count's first with
    two spans, 2T*4096 + 1 k_mask_compact's first with two iterations and the derive pieces' first with two rounds."""
    out = {str(v): v for v in SMALL + (4095, 4096, 4097)}
    out.update({"T*1024+1": T * 1024 + 1, "T*2048": T * 2048, "T*2048+1": T * 2048 + 1, "T*4096": T * 4096, "T*4096+1": T * 4096 + 1,
                "2T*4096+1": 2 * T * 4096 + 1})
    return out


FORCED_SIZES = ("4097", "T*4096+1", "2T*4096+1")          # both front ends forced, all patterns
PATH_SIZES = ("65", "4097", "T*2048+1", "2T*4096+1")      # float centres, keep-order mesh, single-stream context, strips, short lists


def _edge_positions(n, T):
    """{pattern name: position} of the single-survivor patterns: per front end, a turn edge and a chunk edge from the model's
    geometry for this size (the middle one of the streaming front end's list, the first of the lazy one's, the last of the compact
    one's; the third-turn edge where a chunk has three turns), each with the position before it."""
    out = {}
    for front in ref.FRONTS:
        g = ref.geometry(n, T, front)
        inside = lambda edges: [e for e in edges if 1 < e < n - 1]
        for kind, edges in (("turn", inside(g["third_turn_edges"]) or inside(g["turn_edges"])), ("chunk", inside(g["chunk_edges"]))):
            if edges:
                e = edges[{"stream": len(edges) // 2, "lazy": 0, "compact": -1}[front]]
                out[f"{front}:{kind}-1"] = e - 1
                out[f"{front}:{kind}"] = e
    seen, dedup = set(), {}
    for k, p in out.items():
        if p not in seen and 0 < p < n - 1:
            seen.add(p)
            dedup[k] = p
    return dedup


def pattern_names(n, T):
    if n < 4095:
        return [p for p in SMALL_PATTERNS if n > 1 or p in ("all", "none")]
    names = ["all", "none", "first", "last"] + list(_edge_positions(n, T))
    for front in ref.FRONTS:
        names += [f"{front}:last_chunk", f"{front}:odd_turns"]
    return names + ["rand2", "rand30", "rand95", "mod5", "w64", "w32"]


def pattern(name, n, T):
    """bool [n]: the splats pattern `name` keeps (before the behind set is taken out)."""
    i = np.arange(n, dtype=np.int64)
    P = np.zeros(n, dtype=bool)
    if name == "all":
        P[:] = True
    elif name == "none":
        pass
    elif name == "first":
        P[0] = True
    elif name == "last":
        P[n - 1] = True
    elif name.startswith("rand"):
        P = np.random.default_rng(n * 131 + int(name[4:])).random(n) < int(name[4:]) / 100.0
    elif name == "mod5":
        P = i % 5 == 0
    elif name == "w64":
        P = (i // 64) % 2 == 0
    elif name == "w32":
        P = (i // 32) % 3 == 0
    elif name.endswith(":last_chunk"):
        b, e = ref.geometry(n, T, name.split(":")[0])["last_chunk"]
        P[b:e] = True
    elif name.endswith(":odd_turns"):
        P = ref.turn_index(n, T, name.split(":")[0]) % 2 == 1
    else:
        P[_edge_positions(n, T)[name]] = True
    return P


def behind_set(n, T):
    """bool [n]: the splats mirrored behind the camera - runs of 617 original indexes (no multiple of a nibble, a word, a storage
    block or a turn) every 9 x 617, so whole storage blocks of a keep-order mesh die too; every 7th splat of a tiny scene.  The
    positions the single-survivor patterns need (and the last positions of the short lists) stay in front."""
    i = np.arange(n, dtype=np.int64)
    B = (i // 617) % 9 == 4 if n >= 4095 else i % 7 == 3
    B[[0, n - 1]] = False
    if n >= 4095:
        B[list(_edge_positions(n, T).values())] = False
        B[[n - 1 - s for s in SHORT]] = False
    return B


class Scene:
    pass


def make_scene(n, T, half_cov=False):
    """centres float32 [n, 3], cov float32 [n, 6], rgba uint8 [n, 4], behind bool [n], the camera."""
    from gaussiansplats3d_amd import camera
    rng = np.random.default_rng(7000 + n % 9973)
    cam_pos = np.array(camera.DEMO_POSES["garden"][1], dtype=np.float64)
    look = np.array(camera.DEMO_POSES["garden"][2], dtype=np.float64)
    fwd = (look - cam_pos) / np.linalg.norm(look - cam_pos)
    s = Scene()
    s.count, s.half_cov = n, half_cov
    s.behind = behind_set(n, T)
    depth = rng.uniform(2.0, 8.0, size=n).astype(np.float32)
    depth[s.behind] *= np.float32(-1.0)
    lateral = np.clip(rng.standard_normal(size=(n, 3), dtype=np.float32) * np.float32(0.05), -0.15, 0.15)
    s.centers = (cam_pos.astype(np.float32) + depth[:, None] * fwd.astype(np.float32) + lateral).astype(np.float32)
    s.cov = np.zeros((n, 6), dtype=np.float32)
    s.cov[:, [0, 3, 5]] = np.float32(9e-4)
    s.rgba = rng.integers(1, 256, size=(n, 4), dtype=np.uint8)
    s.cam = camera.demo_camera("garden", W, H)
    return s


def oracle_visible(scene, P, visible=(1, 0)):
    """The raster oracle's verdict on the scene under pattern P: bool [n]."""
    import oracle
    cam = scene.cam
    ocam = oracle.set_scenes(oracle.make_camera(cam.model_view(), cam.projection, cam.position, W, H, 0, 0), opacity=[1.0, 1.0],
                             visible=list(visible), effects=True)
    cov = scene.cov
    if scene.half_cov:
        from gaussiansplats3d_amd.util import to_half_three
        cov = to_half_three(cov).view(np.float16).astype(np.float32)
    return oracle.project(ocam, scene.centers, cov, scene.rgba, None, scene_indexes=(~P).astype(np.uint32))["visible"].astype(bool)


# ----------------------------------------------------------------------------------------------------------------- the device rig
class Rig:
    """One mesh and one sorter for a size and a path (context, centre format, storage order); patterns change the scene indexes only."""

    def __init__(self, ctx, n, T, float_centres=False, keep_order=False, half_cov=False, sorter_count=None):
        import oracle
        from gaussiansplats3d_amd import SplatMesh, create_sort_worker, util
        self.n, self.T, self.float_centres = n, T, float_centres
        self.scene = make_scene(n, T, half_cov)
        self.cam = self.scene.cam
        self.mvp = self.cam.sort_mvp()
        self.precision = 20 if float_centres else 16
        self.centres = util.float_centers(self.scene.centers) if float_centres else util.integer_centers(self.scene.centers)
        self.mesh = SplatMesh(ctx, n, 0, half_precision_covariances=half_cov, enable_optional_effects=True, keep_order=keep_order)
        self.P = np.ones(n, dtype=bool)
        self.mesh.build(self.scene.centers, self.scene.cov, self.scene.rgba, scene_indexes=np.zeros(n, dtype=np.uint32))
        self.mesh.set_camera(self.cam)
        self.visible = None
        self.set_visible((1, 0))
        self.sorter_count = n if sorter_count is None else sorter_count       # centres the sorter has received
        m = self.sorter_count
        self.worker = create_sort_worker(ctx, m, integer_based_sort=not float_centres, splat_sort_distance_map_precision=self.precision)
        self.worker.post_message({"centers": self.centres[:m], "range": {"from": 0, "to": m - 1, "count": m}})
        self.worker.sort_on_device(self.mvp, m)
        self.mesh.use_sorter_result(self.worker, m)                            # binds the sorter to the mesh
        self.storage = self.mesh.debug_cull_planes()[2]                        # storage position by original index
        self._oracle, self._expected = oracle, {}
        self.comparisons, self.survivors, self.runs = 0, [], 0

    def set_visible(self, visible):
        if visible != self.visible:
            self.mesh.set_scenes(opacity=[1.0, 1.0], visible=list(visible))
            self.visible = visible

    def set_pattern(self, P):
        if not np.array_equal(P, self.P):
            from gaussiansplats3d_amd import _lib as L
            si = np.ascontiguousarray((~P).astype(np.uint32))          # scene 1 is the hidden one
            L.check(self.mesh.lib.gs_mesh_upload_scene_indexes(self.mesh.handle, 0, self.n, si.ctypes.data))
            self.P = P.copy()

    def want(self, complement=False):
        return (~self.P if complement else self.P) & ~self.scene.behind

    def expected(self, R):
        """(the oracle's sorted list of the first R positions, (key min, key max) over all of them) - once per R."""
        if R not in self._expected:
            order, _, _, lohi, _ = self._oracle.sort_indexes(np.arange(R, dtype=np.uint32), self.centres, self.mvp, precision=self.precision,
                                                            use_int=not self.float_centres, return_intermediates=True)
            if len(self._expected) > 3:
                self._expected.clear()
            self._expected[R] = (order, lohi)
        return self._expected[R]

    def block_census(self, want):
        """(storage blocks with no survivor, blocks with some but not all) - a condition on the input, not on the library."""
        per = np.zeros((self.n + 255) // 256, dtype=np.int64)
        np.add.at(per, self.storage[want] >> 8, 1)
        size = np.bincount(self.storage >> 8, minlength=per.shape[0])
        return int((per == 0).sum()), int(((per > 0) & (per < size)).sum())

    def run(self, P, R=None, complement=False, strip=None, frame=None, label="", nothing=False):
        """project -> visibility-culled sort -> draw for pattern P (or its complement among the splats in front) over the first R
        list positions; returns the list of what differed from the expectation (empty: the comparison passed).  nothing: the strip
        is one the column never reaches, so nothing may survive.  Every comparison draws the culled list and compares visible_splats.
        frame: also draw the unculled sort of the same list and compare the two frames - by default always up to FRAME_ALWAYS
        splats; above, where a draw of millions of splats on four tiles costs a quarter of a second, for every fourth comparison
        and whenever nothing survives.  frame=False: no draw at all."""
        n = self.n
        self.runs += 1
        draw = frame is not False
        if frame is None:
            frame = n <= FRAME_ALWAYS or self.runs % 4 == 1 or not (P.any() if not complement else True) or nothing
        R = self.sorter_count if R is None else R
        self.set_pattern(P)
        self.set_visible((0, 1) if complement else (1, 0))
        want = self.want(complement) & (not nothing)
        order, lohi = self.expected(R)
        mesh, worker = self.mesh, self.worker
        full = None
        if frame:                                              # the frame of the unculled sort of the same list
            worker.set_visibility_cull(False)
            worker.sort_on_device(self.mvp, R)
            mesh.use_sorter_result(worker, R)
            full, _ = mesh.render(tile_rows=strip)
        worker.set_visibility_cull(True)
        mesh.project(strip)
        reply = worker.post_message({"sort": {"modelViewProj": self.mvp, "splatRenderCount": R, "splatSortCount": R}})
        stats = reply["stats"]
        bits = worker.keep_bits(R)
        bad = []
        exp_list = order[want[order]]
        exp_kept = int(want[:R].sum())
        if not np.array_equal(reply["sortedIndexes"], exp_list):
            got = reply["sortedIndexes"]
            k = min(got.shape[0], exp_list.shape[0])
            d = np.nonzero(got[:k] != exp_list[:k])[0]
            bad.append(f"list: {got.shape[0]} entries for {exp_list.shape[0]}, first difference at {d[:1].tolist()}")
        if int(stats.result_count) != exp_kept:
            bad.append(f"result_count {int(stats.result_count)} for {exp_kept}")
        if not np.array_equal(bits, want[:R]):
            d = np.nonzero(bits != want[:R])[0]
            bad.append(f"keep bits: {d.size} differ, first {d[:5].tolist()}")
        if (int(stats.key_min), int(stats.key_max)) != tuple(lohi):
            bad.append(f"min / max {(int(stats.key_min), int(stats.key_max))} for {tuple(lohi)}")
        if draw:
            mesh.use_sorter_result(worker, R)
            got_frame, st = mesh.render(tile_rows=strip)       # consumes the projection
            if R == n and int(st.visible_splats) != exp_kept:
                bad.append(f"visible_splats {int(st.visible_splats)} for {exp_kept}")
            if frame and not np.array_equal(got_frame, full):
                bad.append("frame differs from the unculled sort's")
        self.comparisons += 1
        self.survivors.append(exp_kept)
        return [f"{label or 'case'} R={R}{' complement' if complement else ''}{f' strip {strip}' if strip else ''}: {b}" for b in bad]

    def close(self):
        self.worker.terminate()
        self.mesh.dispose()


def device_T():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def run_patterns(rig, names, **kw):
    """Every pattern of `names` through rig.run; the failures."""
    bad = []
    for name in names:
        bad += rig.run(pattern(name, rig.n, rig.T), label=name, **kw)
    return bad


def run_strips(rig, names):
    """The centre strip (the full frame's mask, written by the vertex stage's atomics and sorted through the compact front end
    unless one is forced) and a strip the column never reaches (nothing kept), each between full frames."""
    bad = []
    for name in names:
        P = pattern(name, rig.n, rig.T)
        bad += rig.run(P, strip=STRIP, label=name)
        bad += rig.run(P, label=name)
        bad += rig.run(P, strip=FAR_STRIP, nothing=True, label=name)
        bad += rig.run(P, complement=True, label=name)
    return bad


def run_lifecycle(rig):
    """A, complement of A, A; the same around a short list; then a strip projection and a full one.  A word left non-zero or
    wrongly declared clean shows as a spurious survivor of the next step."""
    A = pattern("rand30", rig.n, rig.T)
    bad = []
    for comp in (False, True, False):
        bad += rig.run(A, complement=comp, label="A")
    if rig.n > SHORT[0] + 1:
        bad += rig.run(A, R=rig.n - SHORT[0], label="A short")
        bad += rig.run(A, complement=True, label="A after short")
        bad += rig.run(A, R=rig.n - SHORT[1], complement=True, label="A short")
    bad += rig.run(A, label="A after short")
    bad += rig.run(A, strip=STRIP, complement=True, label="A strip")
    bad += rig.run(A, label="A after strip")
    rig.mesh.project(STRIP)                                    # a projection nobody consumes must not leak into the next
    bad += rig.run(A, complement=True, label="A after an unconsumed strip")
    rig.mesh.project(None)
    bad += rig.run(A, label="A after an unconsumed frame")
    return bad
