"""The case list and the rig of the visibility-culled sort of a DYNAMIC-mode sorter (test_dyn_vis_ref.py on the CPU,
test_gpu_dyn_vis.py, tools/dyn_vis_child.py and test_node_dyn_vis.py on the device): csrc/sorter.hip keys every list position with
the row of its own scene - (modelViewProj * transforms[scene])[2] - in k_minmax_count<true> and k_cull_front<MAP, true>.

The scene is vis_front_cases.make_scene's column (its sizes, its patterns, its behind set, its splat size: nothing is shrunk).
Every splat belongs to one of K = 4 "real" scenes and carries the mesh scene index 2k + hidden on a mesh built with dynamic_mode and
enable_optional_effects: transforms[2k] == transforms[2k + 1], visible = [1, 0, 1, 0, ..], so a pattern is one upload of mesh scene
indexes as in the static rig (and visible = [0, 1, ..] is the complement with no upload).  The sorter gets the index 2k.  The four
transforms move the column's local centres (c = the camera's position, f = its view axis):
  0  the identity: depths 2 .. 8;
  1  a turn about the view axis through c and 1.75 along it: depths 3.75 .. 9.75 - this scene owns the key maximum, and its behind
     set (local depths -8 .. -2) stays behind the camera;
  2  a uniform scale of 1.1 about c (the projected sizes do not change) and 0.1 to the camera's right: depths 2.2 .. 8.8, on screen;
  3  half a turn about the camera's up axis through c and 10 back along f: the whole scene, behind set included, lies 2 .. 18
     behind the camera - it draws nothing and owns the key minimum.
Two layouts: `runs` - scenes back to back, the boundaries inside a lane's four positions, inside a wave's span, on a turn edge and
on a chunk edge of the streaming front end (vis_front_ref.geometry) - and `random`, the scene drawn per splat.  The positions the
single-survivor patterns and the short lists need (vis_front_cases) never belong to scene 3.  `odd_w` gives a tenth of the SORTER'S
centres a w other than 1000 / 1.0 (the mesh does not see it): the ABI takes whatever w the caller uploaded.

Expected: the list is oracle.sort_indexes(.., dynamic=True, scene_indexes, transforms) restricted to `want`, min / max are the
oracle's over every list position, and want = P & drawn, where drawn is oracle.project's `visible` for the whole scene under
oracle.set_scenes(.., dynamic=True, effects=True) - per splat, so the CPU tier checks the identity against the oracle pattern by
pattern and the device rig asks the oracle once per rig."""
import numpy as np

import vis_front_cases as cases
import vis_front_ref as ref

K = 4
LAYOUTS = ("runs", "random")
MODES = ("int", "float")                       # integer centres at precision 16, float centres at 20
BIG_PATTERNS = ("all", "rand30", "stream:turn", "stream:chunk", "none")      # T*2048+1 and T*4096+1
HUGE_PATTERNS = ("rand30", "stream:turn")                                    # 2T*4096+1, no frame
PATH_LABELS = ("4097", "T*2048+1")

# mutations of the KEY model (test_dyn_vis_ref.py); minmax_over_survivors is vis_front_ref's own
KEY_MUTATIONS = ("static_key", "scene0_row", "w_dropped", "w_constant", "scene_at_slot")


def _m16(M):
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64).T).reshape(16)


def camera_frame(cam):
    """(position, right, up, forward) of the camera in world space."""
    V = np.asarray(cam.view, dtype=np.float64).reshape(4, 4).T
    return np.asarray(cam.position, dtype=np.float64), V[0, :3].copy(), V[1, :3].copy(), -V[2, :3].copy()


def real_transforms(cam, variant=0):
    """The K transforms as 4 x 4 math matrices.  variant 1: other angles, offsets and scale with the same roles (the test that changes
    the transforms between two sorts)."""
    c, right, up, f = camera_frame(cam)
    angle, along, scale, side, back = ((0.6, 1.75, 1.1, 0.1, 10.0), (-1.1, 1.5, 1.05, -0.08, 12.0))[variant]
    out = [np.eye(4)]
    Kx = np.array([[0, -f[2], f[1]], [f[2], 0, -f[0]], [-f[1], f[0], 0]])
    R = np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = c - R @ c + along * f
    out.append(M)
    M = np.eye(4); M[:3, :3] *= scale; M[:3, 3] = c * (1.0 - scale) + side * right
    out.append(M)
    R = 2.0 * np.outer(up, up) - np.eye(3)
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = c - R @ c - back * f
    out.append(M)
    return out


def mesh_transforms(cam, variant=0):
    """2K column-major 16-vectors: transforms[2k] == transforms[2k + 1]."""
    return [_m16(M) for M in real_transforms(cam, variant) for _ in (0, 1)]


def protected_positions(n, T):
    """Positions a pattern or a short list relies on to be drawn: they never belong to the scene that draws nothing."""
    p = {0, n - 1}
    if n >= 4095:
        p |= set(cases._edge_positions(n, T).values()) | {n - 1 - s for s in cases.SHORT}
    return sorted(p)


def run_boundaries(n, T):
    """The first positions of the runs of the `runs` layout beyond position 0: one inside a lane's four positions, one inside a
    wave's span of 256 (on a lane's edge), one on a turn edge and one on a chunk edge of the streaming front end (where the size has them),
    and the list's last fifth - at most six runs."""
    if n < 8:
        return list(range(1, n))
    b = {n // 5 // 4 * 4 + 2, n * 4 // 5}
    if n >= 4095:
        g = ref.geometry(n, T, "stream")
        b.add(2 * n // 5 // 256 * 256 + 100)
        for edges in (g["turn_edges"], g["chunk_edges"]):
            if edges:
                b.add(edges[len(edges) * 3 // 5])
    else:
        b |= {2 * n // 5, 3 * n // 5}
    return sorted(v for v in b if 0 < v < n)


def scene_of(n, T, layout):
    """uint32 [n]: the real scene (0 .. K-1) of every splat."""
    if layout == "runs":
        k = np.zeros(n, dtype=np.uint32)
        for r, b in enumerate(run_boundaries(n, T)):
            k[b:] = (r + 1) % K
    else:
        k = np.random.default_rng(9000 + n % 9973).integers(0, K, size=n).astype(np.uint32)
    prot = np.array(protected_positions(n, T))
    k[prot[k[prot] == K - 1]] = 1
    return k


def make_scene(n, T, layout, mode="int", odd_w=False, variant=0):
    """vis_front_cases.make_scene's column with the scene of every splat, the transforms and the sorter's centres."""
    from gaussiansplats3d_amd import util
    s = cases.make_scene(n, T)
    s.layout, s.mode = layout, mode
    s.real = scene_of(n, T, layout)
    s.sorter_scene = (2 * s.real).astype(np.uint32)
    s.transforms = mesh_transforms(s.cam, variant)
    s.precision = 16 if mode == "int" else 20
    s.centres4 = util.integer_centers(s.centers) if mode == "int" else util.float_centers(s.centers)
    if odd_w:                                               # every tenth splat (the first one of a tiny scene)
        i = np.arange(0, n, 10)
        s.centres4[i, 3] = (np.array([1, -3, 7, 2001, 0]) if mode == "int" else np.array([0.5, -2.0, 3.25, 0.0, 1.5]))[(i // 10) % 5]
    return s


def mesh_scene_indexes(s, P):
    return (s.sorter_scene + (~P).astype(np.uint32)).astype(np.uint32)


def oracle_visible(s, P, visible=(1, 0)):
    """The raster oracle's verdict on the scene under pattern P (mesh scene index 2k + hidden): bool [n]."""
    import oracle
    cam = s.cam
    ocam = oracle.set_scenes(oracle.make_camera(cam.model_view(), cam.projection, cam.position, cases.W, cases.H, 0, 0),
                             view_matrix=cam.view, transforms=s.transforms, camera_position=cam.position, opacity=[1.0] * (2 * K),
                             visible=list(visible) * K, dynamic=True, effects=True)
    return oracle.project(ocam, s.centers, s.cov, s.rgba, None, scene_indexes=mesh_scene_indexes(s, P))["visible"].astype(bool)


def oracle_sort(s, R):
    """(list, keys, (lo, hi)) of the sort oracle over the first R positions of the identity list."""
    import oracle
    tr = np.concatenate(s.transforms).astype(np.float32)
    order, keys, _, lohi, _ = oracle.sort_indexes(np.arange(R, dtype=np.uint32), s.centres4, s.cam.sort_mvp(), precision=s.precision,
                                                  use_int=s.mode == "int", dynamic=True, scene_indexes=s.sorter_scene, transforms=tr,
                                                  return_intermediates=True)
    return order, keys, lohi


# ----------------------------------------------------------------------------------------------------------- the key, in numpy
def _trunc_f64_i32(v):
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), -2147483648.0).astype(np.int64).astype(np.int32)


def scene_rows(mvp, transforms):
    """(float32 [S, 4], int32 [S, 4]): (mvp * transform)[2] per scene - fp32, left to right - and its x1000 in double, truncated."""
    m = np.asarray(mvp, dtype=np.float64).astype(np.float32).reshape(16)
    fm = np.empty((len(transforms), 4), dtype=np.float32)
    for sc, t in enumerate(transforms):
        b = np.asarray(t, dtype=np.float64).astype(np.float32).reshape(16)
        for c in range(4):
            acc = m[2] * b[4 * c]
            acc = acc + m[6] * b[4 * c + 1]
            acc = acc + m[10] * b[4 * c + 2]
            fm[sc, c] = acc + m[14] * b[4 * c + 3]
    return fm, _trunc_f64_i32(fm.astype(np.float64) * 1000.0)


def model_keys(s, R, mutation=None, survivors=None):
    """int32 [R]: the dynamic key of every position of the identity list, as csrc/sorter.hip's dynamic_key states it.
    mutation: one of KEY_MUTATIONS; scene_at_slot needs `survivors` (bool [n]) - the key of the j-th survivor is taken with the scene
    index of POSITION j, what a kernel does that reads the index where it writes."""
    assert mutation is None or mutation in KEY_MUTATIONS
    fm, im = scene_rows(s.cam.sort_mvp(), s.transforms)
    c = s.centres4[:R]
    si = s.sorter_scene[:R].astype(np.int64)
    if mutation == "scene0_row":
        si = np.zeros(R, dtype=np.int64)
    if mutation == "scene_at_slot":
        pos = np.nonzero(survivors[:R])[0]
        si = si.copy()
        si[pos] = s.sorter_scene[np.arange(pos.shape[0])]
    if mutation == "static_key":                           # the mvp's own third row, no w
        m = np.asarray(s.cam.sort_mvp(), dtype=np.float64).astype(np.float32).reshape(16)
        r = np.tile(np.array([m[2], m[6], m[10], 0.0], dtype=np.float32), (R, 1))
        r = _trunc_f64_i32(r.astype(np.float64) * 1000.0) if s.mode == "int" else r
    else:
        r = (im if s.mode == "int" else fm)[si]
    w = c[:, 3]
    if mutation == "w_constant":
        w = np.full(R, 1000 if s.mode == "int" else 1.0, dtype=c.dtype)
    if s.mode == "int":
        u = lambda a: a.astype(np.int64) & 0xFFFFFFFF
        k = u(c[:, 0]) * u(r[:, 0]) + u(c[:, 1]) * u(r[:, 1]) + u(c[:, 2]) * u(r[:, 2])
        if mutation not in ("w_dropped", "static_key"):
            k = k + u(w) * u(r[:, 3])
        return (k & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    acc = r[:, 0] * c[:, 0]
    acc = acc + r[:, 1] * c[:, 1]
    acc = acc + r[:, 2] * c[:, 2]
    if mutation not in ("w_dropped", "static_key"):
        acc = acc + r[:, 3] * w
    return _trunc_f64_i32(acc.astype(np.float64) * 4096.0)


# ----------------------------------------------------------------------------------------------------------------- the device rig
class _DynamicWorker:
    """The sort worker as a Viewer in dynamic mode drives it: every `sort` message carries the scenes' transforms."""

    def __init__(self, worker, rig):
        self._w, self._rig = worker, rig

    def __getattr__(self, name):
        return getattr(self._w, name)

    def post_message(self, msg):
        if "sort" in msg:
            msg = {"sort": dict(msg["sort"], transforms=self._rig.sort_transforms)}
        return self._w.post_message(msg)

    def sort_on_device(self, mvp, render_count):
        return self.post_message({"sort": {"modelViewProj": mvp, "splatRenderCount": render_count, "splatSortCount": render_count,
                                           "keepOnDevice": True}})


class DynRig(cases.Rig):
    """vis_front_cases.Rig for a dynamic mesh and a dynamic sorter: run(), run_patterns, run_strips and run_lifecycle are its own;
    the scene, how a pattern reaches the mesh, and the expectation are overridden here."""

    def __init__(self, ctx, n, T, layout="runs", mode="int", keep_order=False, odd_w=False):
        from gaussiansplats3d_amd import SplatMesh, create_sort_worker
        self.n, self.T, self.float_centres = n, T, mode == "float"
        self.scene = make_scene(n, T, layout, mode, odd_w)
        s = self.scene
        self.cam, self.mvp, self.precision, self.centres = s.cam, s.cam.sort_mvp(), s.precision, s.centres4
        self.mesh = SplatMesh(ctx, n, 0, dynamic_mode=True, enable_optional_effects=True, keep_order=keep_order)
        self.P = np.ones(n, dtype=bool)
        self.mesh.build(s.centers, s.cov, s.rgba, scene_indexes=mesh_scene_indexes(s, self.P))
        self.mesh.set_camera(self.cam)
        self.visible = None
        self.set_transforms(0)
        self.sorter_count = n
        inner = create_sort_worker(ctx, n, integer_based_sort=mode == "int", dynamic_mode=True, splat_sort_distance_map_precision=self.precision)
        self.worker = _DynamicWorker(inner, self)
        self.worker.post_message({"centers": self.centres, "sceneIndexes": s.sorter_scene, "range": {"from": 0, "to": n - 1, "count": n}})
        self.worker.sort_on_device(self.mvp, n)
        self.mesh.use_sorter_result(self.worker, n)                            # binds the sorter to the mesh
        self.storage = self.mesh.debug_cull_planes()[2]
        self.comparisons, self.survivors, self.runs = 0, [], 0

    def set_transforms(self, variant):
        """New transforms for the mesh (set_scenes) and for every later sort message; the expectation follows."""
        s = self.scene
        s.transforms = mesh_transforms(self.cam, variant)
        self.sort_transforms = np.concatenate(s.transforms).astype(np.float32)
        self.drawn = oracle_visible(s, np.ones(self.n, dtype=bool))
        self._expected = {}
        vis, self.visible = self.visible or (1, 0), None
        self.set_visible(vis)

    def set_visible(self, visible):
        if visible != self.visible:
            self.mesh.set_scenes(transforms=self.scene.transforms, camera_position=self.cam.position, opacity=[1.0] * (2 * K),
                                 visible=list(visible) * K)
            self.visible = visible

    def set_pattern(self, P):
        if not np.array_equal(P, self.P):
            from gaussiansplats3d_amd import _lib as L
            si = np.ascontiguousarray(mesh_scene_indexes(self.scene, P))
            L.check(self.mesh.lib.gs_mesh_upload_scene_indexes(self.mesh.handle, 0, self.n, si.ctypes.data))
            self.P = P.copy()

    def want(self, complement=False):
        return (~self.P if complement else self.P) & self.drawn

    def expected(self, R):
        if R not in self._expected:
            order, _, lohi = oracle_sort(self.scene, R)
            if len(self._expected) > 3:
                self._expected.clear()
            self._expected[R] = (order, lohi)
        return self._expected[R]


def run_paths(rig, names=("rand30", "mod5")):
    """Strips (the centre one and one the column never reaches), a short list and the mask lifecycle on one rig."""
    bad = cases.run_strips(rig, list(names) if rig.n > 1 else ["all"])
    if rig.n > cases.SHORT[0] + 1:
        bad += cases.run_patterns(rig, ["rand30", "last"], R=rig.n - cases.SHORT[0])
        bad += cases.run_lifecycle(rig)
    return bad
