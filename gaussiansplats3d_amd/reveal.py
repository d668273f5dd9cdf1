"""The scene-reveal state machine of the reference's SplatMesh (src/splatmesh/SplatMesh.js:1172-1220, reset :354-362), in that order,
in double: which radius around the averaged scene centre is visible, and how far the fade-in has come.  Pure host arithmetic (the
CPU tier tests it without a device); the one input that needs the splats - the largest distance of a range of centres from the scene
centre - is fed by the caller (SplatMesh.update_visible_region: the root of gs_mesh_bounds's max_dist_sq).
node/VisibleRegion.mjs states the same machine for the drop-in."""

SCENE_FADEIN_RATE_FAST = 0.012
SCENE_FADEIN_RATE_GRADUAL = 0.003
VISIBLE_REGION_EXPANSION_DELTA = 1


class SceneRevealMode:
    Default, Gradual, Instant = 0, 1, 2


class VisibleRegion:
    """Public fields carry the reference's names in snake case."""

    def __init__(self, scene_fade_in_rate_multiplier=1.0):
        self.scene_fade_in_rate_multiplier = float(scene_fade_in_rate_multiplier)
        self.calculated_scene_center = [0.0, 0.0, 0.0]
        self.final_build = False
        self.visible_region_changing = False
        self.shader_fade_in_complete = 0
        self.reset()

    def reset(self):
        """build(..., preserveVisibleRegion = false) on a non-update build (:356-361)."""
        self.max_splat_distance_from_scene_center = 0.0
        self.visible_region_buffer_radius = 0.0
        self.visible_region_radius = 0.0
        self.visible_region_fade_start_radius = 0.0

    def update(self, since_last_build_only, scene_centers, final_build, max_distance_from):
        """updateVisibleRegion(sinceLastBuildOnly) (:1172-1199).  scene_centers: the scenes' sceneCenter, averaged only when
        since_last_build_only is false; max_distance_from(center) -> the largest |c - center| over the splats the reference's loop
        visits ([lastBuildSplatCount, splatCount) or [0, splatCount)), 0 for none.  Ends, as there, with one Default fade step."""
        self.final_build = bool(final_build)
        if not since_last_build_only:
            avg = [0.0, 0.0, 0.0]
            for c in scene_centers:
                avg = [avg[0] + float(c[0]), avg[1] + float(c[1]), avg[2] + float(c[2])]
            s = 1.0 / len(scene_centers)
            self.calculated_scene_center = [avg[0] * s, avg[1] * s, avg[2] * s]
        d = float(max_distance_from(self.calculated_scene_center))
        if d > self.max_splat_distance_from_scene_center:
            self.max_splat_distance_from_scene_center = d
        if self.max_splat_distance_from_scene_center - self.visible_region_buffer_radius > VISIBLE_REGION_EXPANSION_DELTA:
            self.visible_region_buffer_radius = self.max_splat_distance_from_scene_center
            self.visible_region_radius = max(self.visible_region_buffer_radius - VISIBLE_REGION_EXPANSION_DELTA, 0.0)
        if self.final_build:
            self.visible_region_radius = self.visible_region_buffer_radius = self.max_splat_distance_from_scene_center
        self.update_fade_distance()

    def update_fade_distance(self, scene_reveal_mode=SceneRevealMode.Default):
        """updateVisibleRegionFadeDistance(sceneRevealMode) (:1201-1220)."""
        fast = SCENE_FADEIN_RATE_FAST * self.scene_fade_in_rate_multiplier
        gradual = SCENE_FADEIN_RATE_GRADUAL * self.scene_fade_in_rate_multiplier
        default_rate = fast if self.final_build else gradual
        rate = default_rate if scene_reveal_mode == SceneRevealMode.Default else gradual
        self.visible_region_fade_start_radius = ((self.visible_region_radius - self.visible_region_fade_start_radius) * rate +
                                                 self.visible_region_fade_start_radius)
        percentage = (self.visible_region_fade_start_radius / self.visible_region_buffer_radius
                      if self.visible_region_buffer_radius > 0 else 0)
        complete = percentage > 0.99
        self.shader_fade_in_complete = 1 if (complete or scene_reveal_mode == SceneRevealMode.Instant) else 0
        self.visible_region_changing = not complete

    def state(self):
        """The fields in the order of tests/golden/reveal_kat.json's `fields`."""
        return [self.max_splat_distance_from_scene_center, self.visible_region_buffer_radius, self.visible_region_radius,
                self.visible_region_fade_start_radius, self.visible_region_changing, self.shader_fade_in_complete]
