// VisibleRegion.mjs — the scene-reveal state machine of the reference's SplatMesh (src/splatmesh/SplatMesh.js:1172-1220, reset
// :354-362), in that order, in double: which radius around the averaged scene centre is visible and how far the fade-in has come.
// Pure host arithmetic, no device and no `three`: the one input that needs the splats - the largest distance of a range of centres
// from the scene centre - is fed by the caller (node/SplatMesh.mjs: the root of gs_mesh_bounds's maxDistSq).
// gaussiansplats3d_amd/reveal.py states the same machine for the Python mirror.
export const SCENE_FADEIN_RATE_FAST = 0.012;
export const SCENE_FADEIN_RATE_GRADUAL = 0.003;
export const VISIBLE_REGION_EXPANSION_DELTA = 1;
export const SceneRevealMode = { Default: 0, Gradual: 1, Instant: 2 };

export class VisibleRegion {
  constructor(sceneFadeInRateMultiplier = 1.0) {
    this.sceneFadeInRateMultiplier = sceneFadeInRateMultiplier;
    this.calculatedSceneCenter = [0, 0, 0];
    this.finalBuild = false;
    this.visibleRegionChanging = false;
    this.shaderFadeInComplete = 0;
    this.reset();
  }
  // build(..., preserveVisibleRegion = false) on a non-update build (:356-361)
  reset() {
    this.maxSplatDistanceFromSceneCenter = 0;
    this.visibleRegionBufferRadius = 0;
    this.visibleRegionRadius = 0;
    this.visibleRegionFadeStartRadius = 0;
  }
  // updateVisibleRegion(sinceLastBuildOnly) (:1172-1199).  sceneCenters: the scenes' sceneCenter as [x, y, z], averaged only when
  // sinceLastBuildOnly is false; maxDistanceFrom(center) -> the largest |c - center| over the splats the reference's loop visits
  // ([lastBuildSplatCount, splatCount) or [0, splatCount)), 0 for none.  Ends, as there, with one Default fade step.
  update(sinceLastBuildOnly, sceneCenters, finalBuild, maxDistanceFrom) {
    this.finalBuild = !!finalBuild;
    if (!sinceLastBuildOnly) {
      const avg = [0, 0, 0];
      for (const c of sceneCenters) { avg[0] += c[0]; avg[1] += c[1]; avg[2] += c[2]; }
      const s = 1.0 / sceneCenters.length;
      this.calculatedSceneCenter = [avg[0] * s, avg[1] * s, avg[2] * s];
    }
    const d = maxDistanceFrom(this.calculatedSceneCenter);
    if (d > this.maxSplatDistanceFromSceneCenter) this.maxSplatDistanceFromSceneCenter = d;
    if (this.maxSplatDistanceFromSceneCenter - this.visibleRegionBufferRadius > VISIBLE_REGION_EXPANSION_DELTA) {
      this.visibleRegionBufferRadius = this.maxSplatDistanceFromSceneCenter;
      this.visibleRegionRadius = Math.max(this.visibleRegionBufferRadius - VISIBLE_REGION_EXPANSION_DELTA, 0.0);
    }
    if (this.finalBuild) this.visibleRegionRadius = this.visibleRegionBufferRadius = this.maxSplatDistanceFromSceneCenter;
    this.updateFadeDistance();
  }
  // updateVisibleRegionFadeDistance(sceneRevealMode) (:1201-1220)
  updateFadeDistance(sceneRevealMode = SceneRevealMode.Default) {
    const fast = SCENE_FADEIN_RATE_FAST * this.sceneFadeInRateMultiplier;
    const gradual = SCENE_FADEIN_RATE_GRADUAL * this.sceneFadeInRateMultiplier;
    const defaultRate = this.finalBuild ? fast : gradual;
    const rate = sceneRevealMode === SceneRevealMode.Default ? defaultRate : gradual;
    this.visibleRegionFadeStartRadius = (this.visibleRegionRadius - this.visibleRegionFadeStartRadius) * rate + this.visibleRegionFadeStartRadius;
    const percentage = this.visibleRegionBufferRadius > 0 ? this.visibleRegionFadeStartRadius / this.visibleRegionBufferRadius : 0;
    const complete = percentage > 0.99;
    this.shaderFadeInComplete = (complete || sceneRevealMode === SceneRevealMode.Instant) ? 1 : 0;
    this.visibleRegionChanging = !complete;
  }
  // the fields in the order of tests/golden/reveal_kat.json's `fields`
  state() {
    return [this.maxSplatDistanceFromSceneCenter, this.visibleRegionBufferRadius, this.visibleRegionRadius, this.visibleRegionFadeStartRadius,
            this.visibleRegionChanging, this.shaderFadeInComplete];
  }
}
