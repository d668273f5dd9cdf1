"""Host-side mirror of the reference's SplatMesh render seam, over the HIP engine.

Reference interface (/root/reference/src/splatmesh/SplatMesh.js): ``build`` (:306-405) uploads scene data
(``setupDataTextures`` :637-898), ``updateRenderIndexes(globalIndexes, renderSplatCount)`` (:1228-1235),
``updateUniforms(renderDimensions, focalX, focalY, ortho, zoom, inverseFocalAdjustment)`` (:1248-1280),
``setSplatScale`` / ``setPointCloudModeEnabled`` (:1282-1300); the draw itself is
``renderer.render(splatMesh, camera)`` (src/Viewer.js:1616).  Here ``render`` returns the RGBA8 framebuffer
(row 0 = bottom, GL convention) instead of drawing into a WebGL canvas.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .reveal import SceneRevealMode, VisibleRegion
from .util import distance_uniforms, remove_args, removed_below, to_half_three


class SplatMesh:
    def __init__(self, context, max_splat_count, spherical_harmonics_degree=0, half_precision_covariances=False,
                 antialiased=False, kernel_2d_size=0.3, max_screen_space_splat_size=1024.0, splat_scale=1.0,
                 point_cloud_mode=False, spherical_harmonics_8bit=False, dynamic_mode=False,
                 enable_optional_effects=False, keep_order=False, scene_fade_in_rate_multiplier=1.0, render_mode_2d=False):
        self.ctx = context
        self.lib = context.lib
        self.max_splat_count = int(max_splat_count)
        self.sh_degree = int(spherical_harmonics_degree)
        self.render_mode_2d = bool(render_mode_2d)             # splatRenderMode: SplatRenderMode.TwoD (GS_MESH_SURFEL)
        # (2D mode stores scales and rotations in fp32 whatever halfPrecisionCovariancesOnGPU says, SplatMesh.js:666-675)
        self.half_cov = bool(half_precision_covariances) and not self.render_mode_2d
        self.antialiased = bool(antialiased)
        self.kernel_2d_size = float(kernel_2d_size)
        self.max_screen_space_splat_size = float(max_screen_space_splat_size)
        self.splat_scale = float(splat_scale)
        self.point_cloud_mode = bool(point_cloud_mode)
        self.sh_8bit = bool(spherical_harmonics_8bit)          # sphericalHarmonics8BitMode (compression level 2)
        self.dynamic_mode = bool(dynamic_mode)
        self.enable_optional_effects = bool(enable_optional_effects)
        self.fade_in = None                                    # (sceneCenter, visibleRegionFadeStartRadius) or None
        self.keep_order = bool(keep_order)                     # GS_MESH_KEEP_ORDER: device storage in upload order (no Morton)
        self.scene_transforms = None                           # fp64 column-major 16-vectors of set_scenes (dynamic distance pass)
        self.visible_region = VisibleRegion(scene_fade_in_rate_multiplier)   # the scene reveal (update_visible_region*)
        self.scene_centers = [[0.0, 0.0, 0.0]]                 # the scenes' sceneCenter (update_visible_region)
        self.last_build_splat_count = 0                        # splats the last update_visible_region had seen
        self._scene_of = np.zeros(int(max_splat_count), np.uint32)   # host copy of the scene indexes (compute_bounding_box)
        self.splat_count = 0
        self.render_count = 0
        self._indexes = None          # host indexes from updateRenderIndexes
        self._sorter = None           # or a SortWorker whose result is device resident
        self._cam = L.Camera()
        self.last_status = 0
        self.handle = C.c_void_p()
        L.check(self.lib.gs_mesh_create(context.handle, self.max_splat_count, self.sh_degree,
                                        (L.GS_MESH_COV_HALF if self.half_cov else 0) |
                                        (L.GS_MESH_SH_U8 if self.sh_8bit else 0) |
                                        (L.GS_MESH_KEEP_ORDER if self.keep_order else 0) |
                                        (L.GS_MESH_SURFEL if self.render_mode_2d else 0), C.byref(self.handle)))
        context._adopt(self)

    # -- build / data upload ------------------------------------------------------------------------
    def build(self, centers, covariances, colors, spherical_harmonics=None, start=0, scene_indexes=None,
              covariances_are_half_bits=False, scales=None, rotations=None):
        """fillSplatDataArrays output -> device planes.  covariances: float32 [n,6]; narrowed with
        THREE.DataUtils.toHalfFloat semantics when half_precision_covariances (SplatBuffer.js:469-474).
        covariances_are_half_bits=True (half_precision_covariances meshes only): covariances is uint16 [n,6], half bit patterns
        the caller narrowed, stored as they are - the only way to store an inf or a NaN half, which toHalfFloat clamps away.
        spherical_harmonics: float16 (or uint16 bit patterns) [n, 9|24], coefficient-major RGB triples.
        A render_mode_2d mesh takes scales float32 [n,3] and rotations float32 [n,4] (x, y, z, w; normalised, w >= 0) as
        fillSplatScaleRotationArray returns them, and no covariances: scale z becomes 1 (the scaleOverride of
        SplatMesh.fillSplatDataArrays in 2D mode, SplatMesh.js:1856-1863) and (sx, sy, 1, qx, qy, qz) is what the device stores
        (updateScaleRotationsPaddedData, :1155-1170)."""
        c = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 3)
        n = c.shape[0]
        if self.render_mode_2d:
            if scales is None or rotations is None or covariances is not None:
                raise ValueError("a render_mode_2d mesh is built from scales= and rotations=, without covariances")
            sc = np.array(scales, dtype=np.float32).reshape(n, 3)
            sc[:, 2] = 1.0
            covariances = np.concatenate([sc, np.asarray(rotations, dtype=np.float32).reshape(n, 4)[:, :3]], axis=1)
        elif scales is not None or rotations is not None:
            raise ValueError("scales= / rotations= belong to a render_mode_2d mesh")
        if covariances_are_half_bits:
            if not self.half_cov or np.asarray(covariances).dtype != np.uint16:
                raise ValueError("covariances_are_half_bits needs a half_precision_covariances mesh and a uint16 array")
            cov, cov16 = None, np.ascontiguousarray(covariances).reshape(n, 6)
        else:
            cov = np.ascontiguousarray(covariances, dtype=np.float32).reshape(n, 6)
            cov16 = to_half_three(cov) if self.half_cov else None
        rgba = np.ascontiguousarray(colors, dtype=np.uint8).reshape(n, 4)
        sh = None
        sh8 = None
        ncoef = 9 if self.sh_degree == 1 else 24
        if self.sh_degree > 0 and self.sh_8bit:
            sh8 = np.ascontiguousarray(np.asarray(spherical_harmonics, dtype=np.uint8).reshape(n, ncoef))
        elif self.sh_degree > 0:
            sh = np.ascontiguousarray(spherical_harmonics)
            if sh.dtype != np.uint16:
                sh = sh.astype(np.float16).view(np.uint16)
            sh = np.ascontiguousarray(sh.reshape(n, 9 if self.sh_degree == 1 else 24))
        L.check(self.lib.gs_mesh_upload(self.handle, int(start), n, c.ctypes.data,
                                        None if self.half_cov else cov.ctypes.data,
                                        cov16.ctypes.data if self.half_cov else None, rgba.ctypes.data,
                                        sh.ctypes.data if sh is not None else None))
        if sh8 is not None:
            L.check(self.lib.gs_mesh_upload_sh_u8(self.handle, int(start), n, sh8.ctypes.data))
        if scene_indexes is not None:
            si = np.ascontiguousarray(scene_indexes, dtype=np.uint32).reshape(n)
            L.check(self.lib.gs_mesh_upload_scene_indexes(self.handle, int(start), n, si.ctypes.data))
            self._scene_of[int(start):int(start) + n] = si
        self.splat_count = max(self.splat_count, int(start) + n)
        return self

    def remove(self, ranges, scene_remap=None):
        """gs_mesh_remove: the (from, count) ranges go away on the device, every surviving splat i becomes i - (removed splats
        below i); no data crosses the bus.  A mesh in Morton order accepts only ranges whose borders do not split the span of
        one fresh upload (whole scenes); keep_order meshes accept any.  scene_remap[k]: the new index of scene k - call
        set_scenes for the survivors afterwards.  The last draw, a pending project() and bound sorters' results are forgotten."""
        r, n, m, mc = remove_args(ranges, scene_remap)
        L.check(self.lib.gs_mesh_remove(self.handle, r.ctypes.data if n else None, n, m.ctypes.data if m is not None else None, mc))
        old = self.splat_count
        gone = removed_below(r, old)
        if gone:                                           # the host copy of the scene indexes follows: the pieces between the cuts
            pieces, at = [], 0
            for start, count in r.tolist():
                pieces.append(self._scene_of[at:min(start, old)])
                at = max(at, min(start + count, old))
            so = np.concatenate(pieces + [self._scene_of[at:old]])
            if mc:
                so = np.where(so < mc, m[np.minimum(so, mc - 1)], so)
            self._scene_of[:so.size] = so
            self._scene_of[so.size:old] = 0
            self.splat_count = old - gone
        self.render_count = min(self.render_count, self.splat_count)
        self.last_build_splat_count = min(self.last_build_splat_count, self.splat_count)
        self._indexes = None
        return self

    def reorder(self, frm=0, count=None):
        """gs_mesh_reorder: the Morton runs (one per fresh upload) inside [frm, frm + count) become one run on the device, as if
        the range had arrived by one upload - what a progressive load wants at its final build.  count=None: every uploaded
        splat from frm on.  The numbering stays; the last draw, a pending project() and bound sorters' results are forgotten
        unless the call had nothing to do (count 0, a keep_order mesh, at most one run in the range)."""
        if count is None:
            count = max(self.splat_count - int(frm), 0)
        L.check(self.lib.gs_mesh_reorder(self.handle, int(frm), int(count)))
        return self

    def resize(self, max_splat_count):
        """gs_mesh_resize: the capacity becomes max_splat_count (>= splat_count), larger or smaller, on the device - the planes
        are copied there, nothing crosses the bus, and the mesh then behaves as a fresh one of that capacity that received the
        same uploads.  What adding a scene to a live mesh needs: resize, then build(..., start=splat_count).  The last draw, a
        pending project() and bound sorters' results are forgotten unless the capacity is the one the mesh has."""
        n = int(max_splat_count)
        L.check(self.lib.gs_mesh_resize(self.handle, n))
        if n != self.max_splat_count:
            scene_of = np.zeros(n, np.uint32)                  # the host copy of the scene indexes follows
            keep = min(n, self.max_splat_count)
            scene_of[:keep] = self._scene_of[:keep]
            self._scene_of, self.max_splat_count = scene_of, n
        return self

    def set_scenes(self, transforms=None, camera_position=None, opacity=None, visible=None, sh8_range=None):
        """Per-scene uniforms: uniforms.transforms (dynamicMode), sceneOpacity / sceneVisibility
        (enableOptionalEffects), sphericalHarmonics8BitCompressionRangeMin/Max.  transforms: column-major 16-vectors;
        inverse(transform) * cameraPosition (the dynamic-mode SH view origin) is evaluated here in fp64."""
        n = max(len(x) for x in (transforms, opacity, visible, sh8_range) if x is not None)
        if transforms is not None:
            self.scene_transforms = [np.asarray(t, np.float64).reshape(16) for t in transforms]
        sp = L.SceneParams()
        sp.scene_count = n
        for s_ in range(n):
            t = np.eye(4).T.reshape(16) if transforms is None else np.asarray(transforms[s_], np.float64).reshape(16)
            sp.transforms[s_][:] = t.astype(np.float32).tolist()
            if camera_position is not None:
                p = np.linalg.inv(t.reshape(4, 4).T) @ np.array([*np.asarray(camera_position, np.float64), 1.0])
                sp.inv_cam_pos[s_][:] = [*p[:3].astype(np.float32).tolist(), 1.0]
            sp.opacity[s_] = 1.0 if opacity is None else float(min(max(opacity[s_], 0.0), 1.0))     # clamp(), SplatMesh.js:1271
            sp.visible[s_] = 1 if visible is None else int(bool(visible[s_]))
            if sh8_range is not None:
                sp.sh8_min[s_], sp.sh8_max[s_] = float(sh8_range[s_][0]), float(sh8_range[s_][1])
        L.check(self.lib.gs_mesh_set_scenes(self.handle, C.byref(sp)))
        return self

    def compute_distances_on_gpu(self, model_view_proj, out=None, sort_worker=None, integer=None, dynamic=None,
                                 scene_transforms=None):
        """SplatMesh.computeDistancesOnGPU(modelViewProjMatrix, outComputedDistances) (SplatMesh.js:1701-1814): the distance
        pass of gpuAcceleratedSort over every uploaded splat (gs_mesh_compute_distances).  The uniforms are computed here with
        the reference's fp64 arithmetic (getIntegerMatrixArray, per-scene mvp * transform in dynamic mode).
          out          int32 / float32 array of >= uploaded splats, filled by original splat index; None = no host copy
          sort_worker  a SortWorker that receives the distances on the device: sort them with
                       ``post_message({"sort": {..., "usePrecomputedDistances": True, "precomputedOnDevice": True}})``
          integer      integerBasedDistancesComputation (default: the worker's integer_based_sort, else True)
          dynamic      dynamicMode (default: this mesh's); scene_transforms default to those of set_scenes
        Returns `out` (or None)."""
        if integer is None:
            integer = sort_worker.integer_based_sort if sort_worker is not None else True
        dynamic = self.dynamic_mode if dynamic is None else bool(dynamic)
        uniforms, scenes = distance_uniforms(model_view_proj, integer, dynamic,
                                             self.scene_transforms if scene_transforms is None else scene_transforms)
        if out is not None:
            if out.dtype != (np.int32 if integer else np.float32) or not out.flags.c_contiguous or out.size < self.splat_count:
                raise ValueError(f"out must be a contiguous {'int32' if integer else 'float32'} array of >= {self.splat_count} values")
        flags = (L.GS_SORT_INTEGER if integer else 0) | (L.GS_SORT_DYNAMIC if dynamic else 0)
        L.check(self.lib.gs_mesh_compute_distances(self.handle, flags, uniforms.ctypes.data, scenes,
                                                   out.ctypes.data if out is not None else None,
                                                   sort_worker.handle if sort_worker is not None else None))
        return out

    def set_fade_in(self, scene_center=None, visible_region_fade_start_radius=0.0):
        """fadeInComplete == 0 with these uniforms (SplatMesh.updateVisibleRegionFadeDistance); None = complete."""
        self.fade_in = None if scene_center is None else (np.asarray(scene_center, np.float32), float(visible_region_fade_start_radius))

    # -- scene bounds and the scene reveal ----------------------------------------------------------
    def bounds(self, start, count, center, transforms=None):
        """gs_mesh_bounds over splats [start, start + count) of the caller's numbering, reduced on the device: {count - splats
        that took part (a NaN component excludes one), min / max - float32 [3] box of the centres, max_dist_sq - the largest
        |c - center|^2 in fp64, every operation rounded on its own in three.js's order}.  transforms (column-major 16-vectors,
        one per scene): applied to every centre first as THREE.Vector3.applyMatrix4 does, by the splat's scene index."""
        c = (C.c_double * 3)(*[float(v) for v in center])
        out = L.Bounds()
        t, flags = None, 0
        if transforms is not None:
            t = np.ascontiguousarray(np.asarray(transforms, np.float64).reshape(-1, 16))
            flags = L.GS_BOUNDS_TRANSFORM
        L.check(self.lib.gs_mesh_bounds(self.handle, int(start), int(count), C.cast(c, C.c_void_p),
                                        t.ctypes.data if t is not None else None, t.shape[0] if t is not None else 0, flags,
                                        C.byref(out)))
        return {"count": int(out.count), "min": np.array(out.box_min[:], np.float32), "max": np.array(out.box_max[:], np.float32),
                "max_dist_sq": float(out.max_dist_sq)}

    def compute_bounding_box(self, apply_scene_transforms=False, scene_index=None):
        """SplatMesh.computeBoundingBox(applySceneTransforms, sceneIndex) (SplatMesh.js:2066-2095) -> (min, max) float32 [3], over
        the whole mesh or the splats of one scene.  This mirror holds no splat buffers: a static mesh stores the centres its
        caller's fill produced and their box is returned whatever apply_scene_transforms says; a dynamic_mode mesh stores
        untransformed centres and applies the transforms of set_scenes when asked to."""
        start, count = 0, self.splat_count
        if scene_index is not None:
            scenes = max(len(self.scene_transforms or ()), int(self._scene_of[:self.splat_count].max(initial=0)) + 1)
            if scene_index < 0 or scene_index >= scenes:
                raise ValueError("SplatMesh::computeBoundingBox() -> Invalid scene index.")
            own = np.flatnonzero(self._scene_of[:self.splat_count] == scene_index)       # a scene's splats are consecutive
            start, count = (int(own[0]), int(own.size)) if own.size else (0, 0)
        moved = apply_scene_transforms and self.dynamic_mode and self.scene_transforms is not None
        b = self.bounds(start, count, (0.0, 0.0, 0.0), self.scene_transforms if moved else None)
        return b["min"], b["max"]

    def update_visible_region(self, since_last_build_only=False, scene_centers=None, final_build=False):
        """SplatMesh.updateVisibleRegion(sinceLastBuildOnly) (SplatMesh.js:1172-1199), called after a build as the reference's
        refreshDataTexturesFromSplatBuffers does: the largest distance from the averaged scene centre over the splats uploaded
        since the last call (or over all of them) comes from the device (``bounds``); the radii follow in ``visible_region``.
        scene_centers: the scenes' sceneCenter (kept from the last call when omitted)."""
        if scene_centers is not None:
            self.scene_centers = [[float(v) for v in c] for c in scene_centers]
        start = self.last_build_splat_count if since_last_build_only else 0
        transforms = self.scene_transforms if self.dynamic_mode else None

        def max_distance_from(center):
            return float(np.sqrt(self.bounds(start, self.splat_count - start, center, transforms)["max_dist_sq"]))
        self.visible_region.update(since_last_build_only, self.scene_centers, final_build, max_distance_from)
        self.last_build_splat_count = self.splat_count
        return self.visible_region

    def update_visible_region_fade_distance(self, scene_reveal_mode=SceneRevealMode.Default):
        """SplatMesh.updateVisibleRegionFadeDistance(sceneRevealMode) (SplatMesh.js:1201-1220), once per frame: advances the
        fade-in and sets the fade uniforms of the following ``set_camera`` / ``update_uniforms`` - on while the shader's
        fadeInComplete is 0, off once it is 1."""
        v = self.visible_region
        v.update_fade_distance(scene_reveal_mode)
        if v.shader_fade_in_complete:
            self.set_fade_in(None)
        else:
            self.set_fade_in(v.calculated_scene_center, v.visible_region_fade_start_radius)
        return v

    def get_splat_count(self):
        return self.splat_count

    # -- per-sort / per-frame state -------------------------------------------------------------------
    def update_render_indexes(self, global_indexes, render_splat_count):
        """SplatMesh.updateRenderIndexes: host Uint32Array of sorted global indexes (drawn back to front)."""
        self._indexes = np.ascontiguousarray(global_indexes, dtype=np.uint32)
        self._sorter = None
        self.render_count = int(render_splat_count)

    def use_sorter_result(self, sort_worker, render_splat_count):
        """Device-resident alternative: draw the result the sort worker left in HBM."""
        if sort_worker is not None and getattr(sort_worker, "_bound_mesh", None) is not self:
            # from its next sort on, the worker hands over positions in this mesh's storage order (no per-frame translation)
            L.check(self.lib.gs_sorter_bind_mesh(sort_worker.handle, self.handle))
            sort_worker._bound_mesh = self
        self._sorter = sort_worker
        self._indexes = None
        self.render_count = int(render_splat_count)

    def update_uniforms(self, render_dimensions, focal_x, focal_y, orthographic_mode=False, orthographic_zoom=1.0,
                        inverse_focal_adjustment=1.0, model_view=None, projection=None, camera_position=None,
                        spherical_harmonics_degree=None, view_matrix=None):
        """SplatMesh.updateUniforms + three's built-in modelViewMatrix / projectionMatrix / cameraPosition."""
        cam = self._cam
        cam.ortho_zoom = float(orthographic_zoom)
        cam.width, cam.height = int(render_dimensions[0]), int(render_dimensions[1])
        cam.focal[0], cam.focal[1] = float(focal_x), float(focal_y)
        cam.inv_focal_adj = float(inverse_focal_adjustment)
        cam.splat_scale = self.splat_scale
        cam.kernel2d = self.kernel_2d_size
        cam.max_splat_px = self.max_screen_space_splat_size
        cam.sh_degree = self.sh_degree if spherical_harmonics_degree is None else int(spherical_harmonics_degree)
        cam.flags = ((L.GS_CAM_ANTIALIASED if self.antialiased else 0) | (L.GS_CAM_POINT_CLOUD if self.point_cloud_mode else 0) |
                     (L.GS_CAM_ORTHOGRAPHIC if orthographic_mode else 0) | (L.GS_CAM_DYNAMIC if self.dynamic_mode else 0) |
                     (L.GS_CAM_SCENE_EFFECTS if self.enable_optional_effects else 0) |
                     (L.GS_CAM_FADE_IN if self.fade_in is not None else 0))
        if self.fade_in is not None:
            cam.scene_center[:] = self.fade_in[0].tolist()
            cam.fade_start_radius = self.fade_in[1]
        if view_matrix is not None:
            cam.view_matrix[:] = np.asarray(view_matrix, dtype=np.float64).astype(np.float32).reshape(16).tolist()
        if model_view is not None:
            cam.view[:] = np.asarray(model_view, dtype=np.float64).astype(np.float32).reshape(16).tolist()
        if projection is not None:
            cam.proj[:] = np.asarray(projection, dtype=np.float64).astype(np.float32).reshape(16).tolist()
        if camera_position is not None:
            cam.cam_pos[:] = np.asarray(camera_position, dtype=np.float32).tolist()

    def set_camera(self, camera, focal_adjustment=1.0, mesh_world=None, spherical_harmonics_degree=None):
        """Viewer.updateSplatMesh (src/Viewer.js:651-677) for a camera.PerspectiveCamera."""
        fx, fy = camera.focal(focal_adjustment)
        ortho = bool(getattr(camera, "is_orthographic", False))
        self.update_uniforms((camera.width, camera.height), fx, fy, ortho, getattr(camera, "zoom", 1.0), 1.0 / focal_adjustment,
                             camera.model_view(mesh_world), camera.projection, camera.position,
                             spherical_harmonics_degree, view_matrix=camera.view)

    def set_splat_scale(self, splat_scale=1.0):
        self.splat_scale = float(splat_scale)
        self._cam.splat_scale = self.splat_scale

    def set_point_cloud_mode_enabled(self, enabled):
        self.point_cloud_mode = bool(enabled)

    def strip_shape(self, tile_rows=None):
        cam = self._cam
        rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
        r0, r1 = (0, rows_total) if tile_rows is None else tile_rows
        y0, y1 = r0 * L.GS_TILE, min(r1 * L.GS_TILE, cam.height)
        return max(y1 - y0, 0), cam.width

    def project(self, tile_rows=None):
        """The vertex stage on its own (gs_mesh_project) for the camera set by ``set_camera`` / ``update_uniforms`` and the
        strip `tile_rows`; the next ``render`` with the same camera and strip consumes it instead of projecting again."""
        cam = self._cam
        cam.tile_row_begin, cam.tile_row_end = (0, 0) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        L.check(self.lib.gs_mesh_project(self.handle, C.byref(cam)))

    def render(self, tile_rows=None, out_device_ptr=None, want_stats=True, to_host=True):
        """renderer.render(splatMesh, camera).  Returns (uint8[h,w,4] or None, RenderStats or None).
        tile_rows=(begin,end): render only those 16-px tile rows (multi-GPU strips)."""
        cam = self._cam
        cam.tile_row_begin, cam.tile_row_end = (0, 0) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
        h, w = self.strip_shape(tile_rows)
        out = np.empty((h, w, 4), dtype=np.uint8) if to_host else None
        stats = L.RenderStats() if want_stats else None
        idx = self._indexes
        # GS_WARN_FRAME_TRUNCATED: an earlier asynchronous draw overflowed its entry buffer (buffers grown since)
        self.last_status = L.check(self.lib.gs_mesh_render(
            self.handle, C.byref(cam), idx.ctypes.data if idx is not None else None,
            self._sorter.handle if self._sorter is not None else None, self.render_count,
            out.ctypes.data if out is not None else None, C.c_void_p(out_device_ptr) if out_device_ptr else None,
            C.byref(stats) if stats is not None else None))
        return out, stats

    def set_destination(self, depth=None, rgba=None, depth_unorm24=False, depth_device_ptr=None, rgba_device_ptr=None,
                        size=None):
        """What the following draws are depth-tested against and blended over - the reference's `depthTest: true,
        depthWrite: false` + NormalBlending over whatever the host's scene drew first (SplatMaterial3D.js:72-73,
        src/Viewer.js:1610-1616, src/DropInViewer.js:34-42).  depth: float32 [H, W] window depth (row 0 = bottom), rgba: uint8
        [H, W, 4]; or device pointers of the same layouts with size = (width, height).  No arguments: back to a cleared target."""
        if depth is None and rgba is None and depth_device_ptr is None and rgba_device_ptr is None:
            L.check(self.lib.gs_mesh_set_destination(self.handle, None))
            return self
        d = L.Destination()
        keep = []
        if depth is not None and depth_device_ptr:
            raise ValueError("pass the destination depth on the host OR on the device, not both")
        if rgba is not None and rgba_device_ptr:
            raise ValueError("pass the destination colour on the host OR on the device, not both")
        shapes = []                                  # (width, height) every input implies: they must agree
        if size is not None:
            if len(size) != 2:
                raise ValueError("size = (width, height)")
            shapes.append((int(size[0]), int(size[1])))
        if depth is not None:
            a = np.ascontiguousarray(depth, dtype=np.float32)
            if a.ndim != 2:
                raise ValueError("depth must be a float32 array of shape [H, W], got %r" % (a.shape,))
            shapes.append((a.shape[1], a.shape[0]))
            d.depth_host = a.ctypes.data
            keep.append(a)
        if rgba is not None:
            a = np.ascontiguousarray(rgba, dtype=np.uint8)
            if a.ndim != 3 or a.shape[2] != 4:
                raise ValueError("rgba must be a uint8 array of shape [H, W, 4], got %r" % (a.shape,))
            shapes.append((a.shape[1], a.shape[0]))
            d.rgba_host = a.ctypes.data
            keep.append(a)
        if not shapes:
            raise ValueError("device pointers need size = (width, height)")
        if any(sh != shapes[0] for sh in shapes):
            raise ValueError("the destination's depth, colour and size disagree: %r" % (shapes,))
        size = shapes[0]
        if depth_device_ptr:
            d.depth_dev = int(depth_device_ptr)
        if rgba_device_ptr:
            d.rgba_dev = int(rgba_device_ptr)
        d.width, d.height = int(size[0]), int(size[1])
        d.flags = L.GS_DEST_DEPTH_UNORM24 if depth_unorm24 else 0
        L.check(self.lib.gs_mesh_set_destination(self.handle, C.byref(d)))
        return self

    def debug_set_entry_capacity(self, capacity):
        """Test hook: resize the entry buffers (the overflow -> regrow path of a draw)."""
        L.check(self.lib.gs_mesh_debug_set_entry_capacity(self.handle, int(capacity)))

    def last_stats(self):
        stats = L.RenderStats()
        L.check(self.lib.gs_mesh_last_stats(self.handle, C.byref(stats)))
        return stats

    def kernel_time(self, which=0, reset=True):
        """(summed device ms, launches) of one kernel since the last reset; which 0 = k_project."""
        total, n = C.c_double(0.0), C.c_uint32(0)
        L.check(self.lib.gs_mesh_kernel_time(self.handle, int(which), 1 if reset else 0, C.byref(total), C.byref(n)))
        return float(total.value), int(n.value)

    def debug_records(self, count=None):
        """Vertex-stage outputs of the last draw: (records uint32 [n,8], rects uint32 [n,2], visible bool [n]).
        Records and rects are only defined where `visible` is set."""
        n = self.splat_count if count is None else count
        recs = np.empty((n, 8), dtype=np.uint32)
        rects = np.empty((n, 2), dtype=np.uint32)
        words = (n + 63) // 64
        mask = np.empty(words, dtype=np.uint64)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 0, recs.ctypes.data, n))
        L.check(self.lib.gs_mesh_debug_read(self.handle, 1, rects.ctypes.data, n))
        L.check(self.lib.gs_mesh_debug_read(self.handle, 3, mask.ctypes.data, words))
        vis = np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].astype(bool)
        return recs, rects, vis

    def debug_records_2d(self, count=None):
        """Vertex-stage outputs of the last draw of a render_mode_2d mesh: (records uint32 [n,20] - as float32: vT rows Tu, Tv, Tw
        [0:9], vQuadCenter [9:11], the quad's centre in pixels [11:13], the inverse of its 2x2 pixel basis [13:17]; then r|g<<16,
        b|a<<16 (unorm16) and an unused word -, rects uint32 [n,2], visible bool [n]); defined where `visible` is set."""
        n = self.splat_count if count is None else count
        recs = np.empty((n, 20), dtype=np.uint32)
        rects = np.empty((n, 2), dtype=np.uint32)
        words = (n + 63) // 64
        mask = np.empty(words, dtype=np.uint64)
        L.check(self.lib.gs_mesh_debug_read(self.handle, L.GS_DEBUG_RECORDS_2D, recs.ctypes.data, n))
        L.check(self.lib.gs_mesh_debug_read(self.handle, 1, rects.ctypes.data, n))
        L.check(self.lib.gs_mesh_debug_read(self.handle, 3, mask.ctypes.data, words))
        vis = np.unpackbits(mask.view(np.uint8), bitorder="little")[:n].astype(bool)
        return recs, rects, vis

    def debug_depths(self):
        """The window depth the last draw's destination depth test compared for every splat (gs_mesh_debug_read what = 13 through
        the slots of what = 9): float32 [n] in the caller's numbering, NaN where the splat was not visible.  Needs a draw with a
        destination depth."""
        n = self.splat_count
        slots = np.empty(n, dtype=np.uint32)
        plane = np.empty(self.max_splat_count, dtype=np.float32)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 9, slots.ctypes.data, n))
        L.check(self.lib.gs_mesh_debug_read(self.handle, 13, plane.ctypes.data, self.max_splat_count))
        vis = slots != 0xFFFFFFFF
        out = np.full(n, np.nan, dtype=np.float32)
        out[vis] = plane[slots[vis]]
        return out

    def debug_cull_planes(self):
        """The upload-time planes behind the strip and block culls (gs_mesh_debug_read what = 10 / 11 / 12): (cov_bound float32 [n]
        by original splat index; block_box float32 [blocks, 8] per 256-splat storage block - min xyz, max xyz, largest member
        cov_bound, unused; storage position uint32 [n] by original splat index).  Needs no draw."""
        n = self.splat_count
        blocks = (n + 255) // 256
        bound = np.empty(n, dtype=np.float32)
        boxes = np.empty((blocks, 8), dtype=np.float32)
        pos = np.empty(n, dtype=np.uint32)
        if n:
            L.check(self.lib.gs_mesh_debug_read(self.handle, 10, bound.ctypes.data, n))
            L.check(self.lib.gs_mesh_debug_read(self.handle, 11, boxes.ctypes.data, blocks))
            L.check(self.lib.gs_mesh_debug_read(self.handle, 12, pos.ctypes.data, n))
        return bound, boxes, pos

    def bin_entry_counts(self, tile_rows=None):
        """Entries per list bin of the last draw, shaped [list_rows, lists_x] (`tile_rows`: the strip it drew)."""
        cam = self._cam
        LB = int(self.last_stats().list_bin_px)
        bins_x = (cam.width + LB - 1) // LB
        rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
        r0, r1 = (0, rows_total) if tile_rows is None else tile_rows
        y0, y1 = r0 * L.GS_TILE, min(r1 * L.GS_TILE, cam.height)
        b0, b1 = y0 // LB, (max(y1, y0) + LB - 1) // LB if y1 > y0 else y0 // LB
        rng = np.empty(((b1 - b0) * bins_x, 2), dtype=np.uint32)
        if rng.shape[0]:
            L.check(self.lib.gs_mesh_debug_read(self.handle, 2, rng.ctypes.data, rng.shape[0]))
        cnt = np.where(rng[:, 1] > rng[:, 0], rng[:, 1] - rng[:, 0], 0).astype(np.uint32)   # untouched: (~0, 0)
        return cnt.reshape(b1 - b0, bins_x)

    def bin_lists(self, tile_rows=None, list_bin_px=None):
        """The entry lists of the last draw (`tile_rows`: the strip it drew): (ranges uint32 [lists, 2] - [begin, end) per list bin,
        row-major from the strip's first list-bin row, (~0, 0) = untouched; entries uint32 [D] - the record slots the ranges index,
        every list near -> far; slot_of_splat uint32 [n] - the record slot the vertex stage gave each splat, in the caller's
        numbering, 0xFFFFFFFF = not visible).  list_bin_px: the draw's list-bin edge when asking ``last_stats`` for it is not
        wanted (after an asynchronous draw that overflowed, ``last_stats`` regrows the entry buffers)."""
        cam = self._cam
        LB = int(self.last_stats().list_bin_px) if list_bin_px is None else int(list_bin_px)
        bins_x = (cam.width + LB - 1) // LB
        rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
        r0, r1 = (0, rows_total) if tile_rows is None else tile_rows
        y0, y1 = r0 * L.GS_TILE, min(r1 * L.GS_TILE, cam.height)
        b0, b1 = y0 // LB, (y1 + LB - 1) // LB if y1 > y0 else y0 // LB
        rng = np.empty(((b1 - b0) * bins_x, 2), dtype=np.uint32)
        if rng.shape[0]:
            L.check(self.lib.gs_mesh_debug_read(self.handle, 2, rng.ctypes.data, rng.shape[0]))
        touched = rng[:, 1] > rng[:, 0]
        D = int(rng[touched, 1].max()) if touched.any() else 0            # the lists tile [0, D)
        entries = np.empty(D, dtype=np.uint32)
        if D:
            L.check(self.lib.gs_mesh_debug_read(self.handle, 8, entries.ctypes.data, D))
        slots = np.empty(self.splat_count, dtype=np.uint32)
        if self.splat_count:
            L.check(self.lib.gs_mesh_debug_read(self.handle, 9, slots.ctypes.data, self.splat_count))
        return rng, entries, slots

    def bin_word_narrow(self):
        """Which look-up word the last draw's vertex stage left for its binner (csrc/bin_word.hpp; gs_mesh_debug_read what = 14):
        True = the 4-byte word, False = the 8-byte one (a frame beyond 256 tiles in either direction, $GSPLAT_NO_COMPACT_BIN_WORD)."""
        word = np.zeros(1, dtype=np.uint32)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 14, word.ctypes.data, 1))
        return bool(word[0])

    def blend_bin_stats(self, tile_rows=None):
        """Per 32-px blend bin of the last draw - the full frame, or the strip `tile_rows` it drew: (entries scanned, 2 x (splat,
        quadrant) pairs composited), [bin_rows, bins_x, 2], row 0 = the strip's first bin row."""
        cam = self._cam
        rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
        r0, r1 = (0, rows_total) if tile_rows is None else tile_rows
        y0, y1 = r0 * L.GS_TILE, min(r1 * L.GS_TILE, cam.height)
        bx, by = (cam.width + L.GS_BIN - 1) // L.GS_BIN, (y1 + L.GS_BIN - 1) // L.GS_BIN - y0 // L.GS_BIN
        out = np.zeros((by * bx, 2), dtype=np.uint32)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 4, out.ctypes.data, by * bx))
        return out.reshape(by, bx, 2)

    def set_draw_mode(self, rop8=False, full=False):
        """How the following draws composite: the fp32 front-to-back composite rounded once (default), or - rop8=True - the
        reference's RGBA8 render target as a GPU executes it: back to front, every channel rounded to 8 bits after every splat
        (SplatMaterial3D.js:65-75; gs_mesh_set_draw_mode).  GS_DRAW_ROP8 walks the splats in front of each quadrant's saturation depth
        (T <= 1e-6) - ~4x the fp32 blend; full=True (GS_DRAW_ROP8_FULL) walks every list to its end (~70x)."""
        mode = L.GS_DRAW_FP32 if not rop8 else (L.GS_DRAW_ROP8_FULL if full else L.GS_DRAW_ROP8)
        L.check(self.lib.gs_mesh_set_draw_mode(self.handle, mode))
        return self

    def set_deep_pass(self, enabled):
        """Scheduling only (the pixels do not change): whether very deep bins may be composited by one wave per quadrant and
        chunk instead of by one workgroup."""
        L.check(self.lib.gs_mesh_set_deep_pass(self.handle, 1 if enabled else 0))

    def deep_bins(self):
        """The 32-px bins the last draw composited through the deep pass (one wave per quadrant and chunk; chosen from the
        statistics of the draw before it)."""
        return self.deep_pass_info()["bins"]

    def deep_pass_info(self):
        """{bins drawn by the deep pass, bins over its threshold, chunk partials the per-bin kernel closed itself, whether its
        partial pool ran out} of the last draw."""
        out = np.zeros(4 + 512, dtype=np.uint32)               # 4 words + at most GS_DEEP_MAX_BINS = 512 bins
        L.check(self.lib.gs_mesh_debug_read(self.handle, 5, out.ctypes.data, out.size))
        return {"bins": out[4:4 + int(out[0])].copy(), "candidates": int(out[1]), "chunks_closed_by_bins": int(out[2]),
                "pool_exhausted": bool(out[3])}

    def blend_schedule(self):
        """What the last draw's blend schedule was given and produced (tile_bin.hip blend_schedule_job): {ran, blend_bins, sx, sy
        (this draw's bin (x, y) read the statistics of bin (x - sx, y - sy) of the draw before), deep (this draw ran the deep
        pass), deep_min, deep_factor, order_taken (the blend visited its bins in the schedule's order, else row-major),
        candidates (mirror word 4: bins over the deep pass's trigger, else 0),
        share (mirror word 5: the members' share of the walk in 1/1024), order (the bins in blend order; None when it did not
        run)}.  Scheduling only: frames do not depend on it."""
        head = np.zeros(L.GS_SCHEDULE_WORDS, dtype=np.uint32)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 7, head.ctypes.data, head.size))
        bins = int(head[1]) if head[0] else 0
        out = np.zeros(L.GS_SCHEDULE_WORDS + bins, dtype=np.uint32)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 7, out.ctypes.data, out.size))
        sx, sy = out[2:4].view(np.int32)
        return {"ran": bool(out[0]), "blend_bins": int(out[1]), "sx": int(sx), "sy": int(sy), "deep": bool(out[4]),
                "deep_min": int(out[5]), "deep_factor": int(out[6]), "order_taken": bool(out[7] & 1), "candidates": int(out[8]),
                "share": int(out[9]), "order": out[L.GS_SCHEDULE_WORDS:].copy() if out[0] else None}

    def view_share(self):
        """{visible, projected: of the last full-frame draw whose verdict has reached the host (a mapped word, no statistics call
        needed), block_test: where the last vertex stage ran its block test - 1 a kernel of its own, 0 in every workgroup, 2 nowhere,
        instance: the k_project instance it launched - bit 0 the shader-permutation kernel, bit 1 window depths written, bit 2 the
        4-byte look-up word}.  Scheduling only: frames do not depend on it."""
        out = np.zeros(4, dtype=np.uint32)
        L.check(self.lib.gs_mesh_debug_read(self.handle, 6, out.ctypes.data, 4))
        return {"visible": int(out[0]), "projected": int(out[1]), "block_test": int(out[2]), "instance": int(out[3])}

    def tile_row_costs(self):
        """Work estimate per 16-px tile row of the last FULL-frame draw (used to balance multi-GPU strips).  The blend is
        what a strip mostly pays for and its cost is what it WALKS before its pixels saturate, not the length of its lists:
        per 32-px bin row, the half tiles it evaluated (0.55 of a whole-tile walk each) + an eighth of the entries it staged;
        binning / entry sorting add the list entries of the row (a quarter each).  Rows inherit an even share of the bin /
        list-bin row they lie in."""
        cam = self._cam
        rows_total = (cam.height + L.GS_TILE - 1) // L.GS_TILE
        ratio = int(self.last_stats().list_bin_px) // L.GS_TILE
        entries = np.repeat(self.bin_entry_counts().sum(axis=1).astype(np.float64) / ratio, ratio)[:rows_total]
        st = self.blend_bin_stats().astype(np.float64).sum(axis=1)          # [bin_rows, 2]
        blend = np.repeat((0.55 * st[:, 1] + st[:, 0] / 8.0) / 2.0, 2)[:rows_total]
        if blend.shape[0] < rows_total:
            blend = np.pad(blend, (0, rows_total - blend.shape[0]))
        return blend + 0.25 * entries

    def rop8_window(self, x0, y0, width, height):
        """Verification: the window [x0, x0+width) x [y0, y0+height) of the LAST draw composited the reference's way - back to
        front into an RGBA8 target, every channel rounded to 8 bits after every splat (gs_mesh_debug_rop8;
        SplatMaterial3D.js:65-75).  uint8 [height, width, 4], row 0 = y0 (GL orientation)."""
        out = np.empty((int(height), int(width), 4), dtype=np.uint8)
        L.check(self.lib.gs_mesh_debug_rop8(self.handle, int(x0), int(y0), int(width), int(height), out.ctypes.data))
        return out

    def surface(self, x0, y0, width, height, threshold=0.5, ids_device_ptr=None, depth_device_ptr=None):
        """Where the splat surface of the LAST draw is (gs_mesh_surface): per pixel of the window [x0, x0+width) x [y0, y0+height)
        (GL window coordinates, row 0 = bottom) the first splat of the pixel's near -> far list after which the transmittance
        T = prod(1 - alpha) has fallen to `threshold`, and the window depth of that splat's centre.  Returns (ids uint32 [h, w] -
        the caller's splat numbering, 0xFFFFFFFF = the list ends first; depth float32 [h, w] - 0.5 * ndc.z + 0.5, 1.0 = none).
        A plane given as a device pointer (uint32 / float32 [h, w]) is only enqueued on the context's stream and comes back as
        None.  ``camera.unproject`` with the camera's view matrix turns (px + 0.5, py + 0.5, depth) into the world point."""
        h, w = int(height), int(width)
        ids = None if ids_device_ptr else np.empty((max(h, 0), max(w, 0)), dtype=np.uint32)
        depth = None if depth_device_ptr else np.empty((max(h, 0), max(w, 0)), dtype=np.float32)
        L.check(self.lib.gs_mesh_surface(self.handle, int(x0), int(y0), w, h, float(threshold),
                                         ids.ctypes.data if ids is not None else None,
                                         depth.ctypes.data if depth is not None else None,
                                         C.c_void_p(int(ids_device_ptr)) if ids_device_ptr else None,
                                         C.c_void_p(int(depth_device_ptr)) if depth_device_ptr else None))
        return ids, depth

    def dispose(self):
        if self.handle:
            self.lib.gs_mesh_destroy(self.handle)
            self.handle = C.c_void_p()

    close = dispose

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass
