/* oracle/texel_pack.h — TEST INFRASTRUCTURE.  The data-texture texel packing of the reference's SplatMesh.setupDataTextures
 * (src/splatmesh/SplatMesh.js:637-898), shared by the two harnesses that run the reference's shader text:
 * oracle/shader_harness.cpp (CPU, glsl_shim.hpp) and oracle/gl_ref.c (a real GLES 3 sampler).  One packer, two texture
 * layouts: the caller chooses the texture's width and height (in texels) and owns the buffer; every function fills the whole
 * buffer (padding texels zero), so a texel's position only depends on its linear index.
 *
 * Texel packing, per texture (elements per texel / per splat as SplatMesh.js:19-28 declares them):
 *   centersColors    RGBA32UI  one texel per splat: {rgba8 packed little-endian (Util.js rgbaArrayToInteger), bits(x), bits(y),
 *                              bits(z)} (updateCenterColorsPaddedData, :1143-1153)
 *   covariances      RGBA32F   6 floats per splat back to back, 1.5 texels per splat (covariancesTextureData.set, :729)
 *   covariancesHalf  RGBA32UI  one texel per splat: 3 uint32 of two IEEE halves each (low half first), the 4th word zero
 *                              (updatePaddedCompressedCovariancesTextureData, :1127-1141)
 *   sphericalHarmonics         `stride` components per splat back to back (9 -> 10 and 24 -> 24 padded, :797-805), 4 per texel
 *   sceneIndexes     R32UI     one texel per splat (:881-886)
 */
#ifndef GS_ORACLE_TEXEL_PACK_H
#define GS_ORACLE_TEXEL_PACK_H

#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

static inline size_t tp_texels(int w, int h) { return (size_t)w * (size_t)h; }

/* dst: uint32[4 * w * h] */
static inline void tp_pack_centers_colors(uint32_t n, const float* centers, const uint8_t* rgba, int w, int h, uint32_t* dst) {
    memset(dst, 0, sizeof(uint32_t) * 4 * tp_texels(w, h));
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* c = rgba + 4 * (size_t)i;
        dst[4 * (size_t)i] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
        memcpy(&dst[4 * (size_t)i + 1], centers + 3 * (size_t)i, 12);
    }
}

/* dst: float[4 * w * h]; needs 6 n <= 4 w h */
static inline void tp_pack_covariances(uint32_t n, const float* cov, int w, int h, float* dst) {
    memset(dst, 0, sizeof(float) * 4 * tp_texels(w, h));
    memcpy(dst, cov, sizeof(float) * 6 * (size_t)n);
}

/* dst: uint32[4 * w * h]; cov16: IEEE-half bits [6 n] */
static inline void tp_pack_covariances_half(uint32_t n, const uint16_t* cov16, int w, int h, uint32_t* dst) {
    memset(dst, 0, sizeof(uint32_t) * 4 * tp_texels(w, h));
    for (uint32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++)
            dst[4 * (size_t)i + k] = (uint32_t)cov16[6 * (size_t)i + 2 * k] | ((uint32_t)cov16[6 * (size_t)i + 2 * k + 1] << 16);
}

/* The padded component count of one splat's SH block (9 -> 10, 24 -> 24). */
static inline uint32_t tp_sh_stride(uint32_t ncoef) { return ncoef % 2 ? ncoef + 1 : ncoef; }

/* dst: float[4 * w * h]; sh: [ncoef n] as the sampler returns them */
static inline void tp_pack_sh(uint32_t n, uint32_t ncoef, const float* sh, int w, int h, float* dst) {
    const uint32_t stride = tp_sh_stride(ncoef);
    memset(dst, 0, sizeof(float) * 4 * tp_texels(w, h));
    for (uint32_t i = 0; i < n; i++) memcpy(&dst[(size_t)i * stride], sh + (size_t)i * ncoef, sizeof(float) * ncoef);
}

/* dst: uint32[w * h] */
static inline void tp_pack_scene_indexes(uint32_t n, const uint32_t* scene_idx, int w, int h, uint32_t* dst) {
    memset(dst, 0, sizeof(uint32_t) * tp_texels(w, h));
    memcpy(dst, scene_idx, sizeof(uint32_t) * (size_t)n);
}

#ifdef __cplusplus
}
#endif
#endif
