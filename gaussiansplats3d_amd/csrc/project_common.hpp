// project_common.hpp — what the two vertex stages share (project.hip: the 3D covariance projection; project_2d.hip: the surfel
// projection of SplatRenderMode.TwoD): the mesh planes as a kernel argument, one corner of the block test, the colour helpers and
// the view-dependent colour of the base stage (SplatMaterial.js:179-337).  Text moved out of project.hip unchanged.
#pragma once
#include "gs_internal.hpp"

struct MeshPlanes {
    const float* __restrict__ px;
    const float* __restrict__ py;
    const float* __restrict__ pz;
    const void* __restrict__ covA;      // fp32: float4 (c0..c3)   | fp16: uint2 (c0..c3)
    const void* __restrict__ covB;      // fp32: float2 (c4,c5)    | fp16: uint  (c4,c5)
    const float* __restrict__ cov_bound;   // spectral-radius bound of the covariance (mesh.hip, cov_spectral_bound)
    const float* __restrict__ block_box;   // per 256-splat storage block: {min xyz, max xyz, max cov_bound, -} (mesh.hip, k_block_boxes)
    const uint32_t* __restrict__ rgba;
    const uint4* __restrict__ sh0;      // halfs 0..7
    const void* __restrict__ sh1;       // SH2: uint4 halfs 8..15 | SH1: uint (half 8)
    const uint4* __restrict__ sh2;      // SH2: halfs 16..23
    const uint32_t* __restrict__ scene_idx;          // per-splat scene (EXT, scene_count > 1)
    const gs_scene_params* __restrict__ scenes;      // per-scene uniforms (EXT)
};

// One storage block's verdict: can NO splat of the block reach the frame (or this rank's strip)?  See k_project's header comment
// for the argument; `corner` evaluates one of the box's eight corners, the reductions over the corners are the caller's.
struct BlockCorner {
    float q[4], v[3];
    bool rej[6];            // this corner satisfies reject k (x > 1.2 w, x < -1.2 w, y > .., y < .., z < -1.2 w, w < 0) beyond the margin
    bool front;             // properly in front of the camera
    float ypx;              // its window y
};
__device__ __forceinline__ BlockCorner block_corner(const ProjectParams& pp, const float* bb, uint32_t c) {
    BlockCorner o;
    const float x = (c & 1u) ? bb[3] : bb[0], y = (c & 2u) ? bb[4] : bb[1], z = (c & 4u) ? bb[5] : bb[2];
    const float* MV = pp.view;
    const float* P = pp.proj;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = MV[r] * x + MV[4 + r] * y + MV[8 + r] * z + MV[12 + r];
#pragma unroll
    for (int r = 0; r < 4; r++) o.q[r] = P[r] * v[0] + P[4 + r] * v[1] + P[8 + r] * v[2] + P[12 + r] * v[3];
    o.v[0] = v[0]; o.v[1] = v[1]; o.v[2] = v[2];
    const float clip = 1.2f * o.q[3], tol = 1e-4f * (fabsf(o.q[0]) + fabsf(o.q[1]) + fabsf(o.q[2]) + fabsf(clip) + 1.0f);
    o.rej[0] = o.q[0] - clip > tol; o.rej[1] = -o.q[0] - clip > tol;
    o.rej[2] = o.q[1] - clip > tol; o.rej[3] = -o.q[1] - clip > tol;
    o.rej[4] = -o.q[2] - clip > tol; o.rej[5] = -o.q[3] > tol;
    o.front = o.q[3] > 1e-6f && v[2] < -1e-6f;
    o.ypx = (o.q[1] / o.q[3] * 0.5f + 0.5f) * pp.height;
    return o;
}

__device__ __forceinline__ float h2f(uint32_t bits16) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(bits16 & 0xFFFFu));
}
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
__device__ __forceinline__ uint32_t unorm16(float v) { return (uint32_t)(clamp01(v) * 65535.0f + 0.5f); }

constexpr uint32_t RECT_EMPTY_LO = 0x0000FFFFu;   // x0 = 0xFFFF > x1 = 0 -> zero tiles

struct ShPre {                  // fp16 SH planes fetched together with the covariance (GS_SH_EARLY): one dependent round trip less
    uint4 a, b, c;
    bool have;
};
template <bool EXT>
__device__ __forceinline__ void sh_colour(const ProjectParams& pp, const MeshPlanes& mp, uint32_t i, uint32_t scene, float c0,
                                          float c1, float c2, float* col, const ShPre& pre) {
    if (pp.sh_stored >= 1 && pp.sh_degree >= 1) {
        float cp0 = pp.cam_pos[0], cp1 = pp.cam_pos[1], cp2 = pp.cam_pos[2];
        if (EXT && (pp.flags & GS_CAM_DYNAMIC)) {                // :179-183 camera in the scene's own frame
            cp0 = mp.scenes->inv_cam_pos[scene][0]; cp1 = mp.scenes->inv_cam_pos[scene][1];
            cp2 = mp.scenes->inv_cam_pos[scene][2];
        }
        float d0 = c0 - cp0, d1 = c1 - cp1, d2 = c2 - cp2;                                 // :185
        const float inv = 1.0f / sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
        const float x = d0 * inv, y = d1 * inv, z = d2 * inv;
        float sh[24];
        const uint4 a = pre.have ? pre.a : mp.sh0[i];
        if (EXT && pp.sh_u8) {
            // 8-bit SH (:150-154,265-269): texel = v/255 (unorm8), sh = texel*range + min; sh0 = bytes 0..15
            const float mn = mp.scenes->sh8_min[scene], range = mp.scenes->sh8_max[scene] - mn;
            const uint32_t w0[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int k = 0; k < 16; k++) sh[k] = ((float)((w0[k >> 2] >> (8 * (k & 3))) & 255u) / 255.0f) * range + mn;
            if (pp.sh_stored >= 2) {
                const uint2 b = reinterpret_cast<const uint2*>(mp.sh1)[i];
                const uint32_t w1[2] = {b.x, b.y};
#pragma unroll
                for (int k = 0; k < 8; k++) sh[16 + k] = ((float)((w1[k >> 2] >> (8 * (k & 3))) & 255u) / 255.0f) * range + mn;
            }
        } else {
        sh[0] = h2f(a.x); sh[1] = h2f(a.x >> 16); sh[2] = h2f(a.y); sh[3] = h2f(a.y >> 16);
        sh[4] = h2f(a.z); sh[5] = h2f(a.z >> 16); sh[6] = h2f(a.w); sh[7] = h2f(a.w >> 16);
        if (pp.sh_stored >= 2) {
            const uint4 b = pre.have ? pre.b : reinterpret_cast<const uint4*>(mp.sh1)[i];
            sh[8] = h2f(b.x); sh[9] = h2f(b.x >> 16); sh[10] = h2f(b.y); sh[11] = h2f(b.y >> 16);
            sh[12] = h2f(b.z); sh[13] = h2f(b.z >> 16); sh[14] = h2f(b.w); sh[15] = h2f(b.w >> 16);
        } else {
            sh[8] = h2f(reinterpret_cast<const uint32_t*>(mp.sh1)[i]);
        }
        }
        const float SH_C1 = 0.4886025119029199f;                                            // :273
#pragma unroll
        for (int ch = 0; ch < 3; ch++) col[ch] += SH_C1 * (-sh[0 + ch] * y + sh[3 + ch] * z - sh[6 + ch] * x);
        if (pp.sh_stored >= 2 && pp.sh_degree >= 2) {                                       // :308-330
            if (!(EXT && pp.sh_u8)) {
                const uint4 cc = pre.have ? pre.c : mp.sh2[i];
                sh[16] = h2f(cc.x); sh[17] = h2f(cc.x >> 16); sh[18] = h2f(cc.y); sh[19] = h2f(cc.y >> 16);
                sh[20] = h2f(cc.z); sh[21] = h2f(cc.z >> 16); sh[22] = h2f(cc.w); sh[23] = h2f(cc.w >> 16);
            }
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            const float C0 = 1.0925484f, C1 = -1.0925484f, C2 = 0.3153916f, C3 = -1.0925484f, C4 = 0.5462742f;
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
                col[ch] += (C0 * xy) * sh[9 + ch] + (C1 * yz) * sh[12 + ch] + (C2 * (2.0f * zz - xx - yy)) * sh[15 + ch] +
                           (C3 * xz) * sh[18 + ch] + (C4 * (xx - yy)) * sh[21 + ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) col[ch] = clamp01(col[ch]);                          // :337
    }
}

// The surfel kernel's launch (project_2d.hip), on ctx->aux: gs_launch_project hands a GS_MESH_SURFEL mesh on to it where it would
// launch k_project - behind the mask preparation and k_block_test, inside the timing events.  block_tested: k_block_test has
// decided (block_any holds its verdicts); else no block is tested at all (per-scene transforms, $GSPLAT_NO_BLOCK_CULL).
int gs_launch_project_2d(gs_mesh* m, const ProjectParams& pp, const MeshPlanes& mp, ProjSet& ps, uint32_t* vis_orig, const uint32_t* inv_perm,
                         bool block_tested);
