// project_2d.hip — vertex stage of a GS_MESH_SURFEL mesh (SplatRenderMode.TwoD): one thread per splat in STORAGE order, one
// 256-splat storage block per workgroup, as k_project.
//
// Restates (never copies) the reference's 2D-Gaussian vertex shader:
//   /root/reference/src/splatmesh/SplatMaterial.js:112-341    the base stage (fetch, per-scene visibility, view / clip transform,
//                                                             1.2x centre reject, SH colour) - the helpers of project_common.hpp
//   /root/reference/src/splatmesh/SplatMaterial2D.js:94-236   scale / rotation -> L = R S, the splat-to-pixel homography T, the
//                                                             eigen-aligned quad and, below one pixel, the reference AABB quad
//                                                             (useRefImplementation = false), then the fade-in (:238)
// in fp32, in the shader's stated operation order (built with -ffp-contract=off, like project.hip).  What the 2D projection text
// does not read - splatScale, kernel2DSize, maxScreenSpaceSplatSize, the antialiased and point-cloud switches, and in this material
// the per-scene OPACITY (only SplatMaterial3D multiplies it in; the visibility reject is the base stage's) - is ignored as it
// ignores it.
//
// The six fp32 values the reference keeps per splat in 2D mode (scale xyz, rotation xyz; SplatMesh.js:666-675, 1155-1170) live in
// the covariance planes: covA = (sx, sy, sz, qx), covB = (qy, qz).
//
// Outputs: tile rect, look-up word, visibility masks and window depth exactly in k_project's layout (the binner, the sorter's
// visibility cull and the statistics read them unchanged), and an 80-byte SurfelRec per survivor slot instead of a SplatRec.
// A splat survives when the shader writes gl_Position, GL does not clip the quad whole (its depth is the centre's), and the quad's
// pixel bounding box holds a pixel centre of the viewport (a superset of "the quad holds one": the blend decides per pixel).
#include "project_common.hpp"

template <bool EXT, bool DEPTH, bool NARROW>
__global__ __launch_bounds__(256) void k_project_2d(ProjectParams pp, MeshPlanes mp, SurfelRec* __restrict__ recs, uint2* __restrict__ rects,
                                                    unsigned long long* __restrict__ vis_mask, uint2* __restrict__ vis32,
                                                    uint32_t* __restrict__ vis_orig, const uint32_t* __restrict__ inv_perm,
                                                    uint8_t* __restrict__ block_any, void* __restrict__ prect, float* __restrict__ zrec,
                                                    uint32_t block_tested) {
    const uint32_t blk = blockIdx.x;
    if (block_tested && block_any[blk] == 0) return;       // k_block_test found the block dead and wrote its empty masks
    const uint32_t i = blk * 256u + threadIdx.x;
    bool visible = false;
    SurfelRec rec = {};
    uint2 rect = make_uint2(RECT_EMPTY_LO, 0u);
    float zwin = 0.0f;

    if (i < pp.count) {
        const float* P = pp.proj;
        const float c0 = mp.px[i], c1 = mp.py[i], c2 = mp.pz[i];
        const float4 sa = reinterpret_cast<const float4*>(mp.covA)[i];
        const float2 sb = reinterpret_cast<const float2*>(mp.covB)[i];
        const uint32_t packed = mp.rgba[i];
        uint32_t scene = 0;
        bool scene_ok = true;
        float MV[16];                     // transformModelViewMatrix, in registers either way (a pointer to one of two arrays costs scratch)
#pragma unroll
        for (int k = 0; k < 16; k++) MV[k] = pp.view[k];
        if (EXT) {
            if (pp.scene_count > 1) scene = mp.scene_idx[i];                          // SplatMaterial.js:123-126
            if (pp.flags & GS_CAM_SCENE_EFFECTS)                                      // :129-137
                scene_ok = !(mp.scenes->opacity[scene] <= 0.01f || mp.scenes->visible[scene] == 0u);
            if (pp.flags & GS_CAM_DYNAMIC) {                                          // :140-144 viewMatrix * transform
                const float* A = pp.view_matrix;
                const float* B = mp.scenes->transforms[scene];
#pragma unroll
                for (int col = 0; col < 4; col++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        MV[4 * col + r] = A[r] * B[4 * col] + A[4 + r] * B[4 * col + 1] + A[8 + r] * B[4 * col + 2] +
                                          A[12 + r] * B[4 * col + 3];
            }
        }
        // SplatMaterial.js:156-166: centre clip test, ndcCenter
        float v[4], q[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = MV[r] * c0 + MV[4 + r] * c1 + MV[8 + r] * c2 + MV[12 + r];
#pragma unroll
        for (int r = 0; r < 4; r++) q[r] = P[r] * v[0] + P[4 + r] * v[1] + P[8 + r] * v[2] + P[12 + r] * v[3];
        const float clip = 1.2f * q[3];
        bool ok = scene_ok && !(q[2] < -clip || q[0] < -clip || q[0] > clip || q[1] < -clip || q[1] > clip);
        const float ndcx = q[0] / q[3], ndcy = q[1] / q[3], ndcz = q[2] / q[3];
        ok = ok && (ndcz >= -1.0f && ndcz <= 1.0f);       // quad z == ndcCenter.z (SplatMaterial2D.js:183, 228): GL clips it whole
        if (DEPTH) {                                      // as k_project: what the destination's depth test compares
            zwin = ndcz * 0.5f + 0.5f;
            if (pp.depth_mode == 2u) zwin = (float)floor((double)zwin * 16777215.0 + 0.5);
        }
        if (ok) {
            float col[3] = {(float)(packed & 255u) * (1.0f / 255.0f), (float)((packed >> 8) & 255u) * (1.0f / 255.0f),
                            (float)((packed >> 16) & 255u) * (1.0f / 255.0f)};                 // SplatMaterial.js:169
            float alpha = (float)(packed >> 24) * (1.0f / 255.0f);
            // SplatMaterial2D.js:96-113  scale, rotation (w rebuilt), L = R * S
            const float s0 = sa.x, s1 = sa.y, s2 = sa.z, qx = sa.w, qy = sb.x, qz = sb.y;
            const float qw = sqrtf(1.0f - qx * qx - qy * qy - qz * qz);
            // quaternionToRotationMatrix (SplatMaterial.js:64-78), columns R0, R1 (R2 only reaches the unused `normal` and a column
            // of Tt that is multiplied by 0)
            const float R0[3] = {1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy + qw * qz), 2.0f * (qx * qz - qw * qy)};
            const float R1[3] = {2.0f * (qx * qy - qw * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz + qw * qx)};
            const float L0[3] = {R0[0] * s0, R0[1] * s0, R0[2] * s0};
            const float L1[3] = {R1[0] * s1, R1[1] * s1, R1[2] * s1};
            (void)s2;
            // :119 world2ndc = transpose(projectionMatrix * transformModelViewMatrix): M[4 k + c] = clip row c of basis vector k
            float M[16];
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    M[4 * k + r] = P[r] * MV[4 * k] + P[4 + r] * MV[4 * k + 1] + P[8 + r] * MV[4 * k + 2] + P[12 + r] * MV[4 * k + 3];
            // :125 X = transpose(splat2World) * world2ndc: X[c][r] = clip coordinate c of splat2World's column r
            // (columns (L0, 0), (L1, 0), (centre, 1): their w terms are 0 * M and 1 * M)
            float X[4][3];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                X[c][0] = L0[0] * M[c] + L0[1] * M[4 + c] + L0[2] * M[8 + c];
                X[c][1] = L1[0] * M[c] + L1[1] * M[4 + c] + L1[2] * M[8 + c];
                X[c][2] = c0 * M[c] + c1 * M[4 + c] + c2 * M[8 + c] + M[12 + c];
            }
            // T = X * ndc2pix (:121-125), ndc2pix = columns (W/2, 0, 0, (W-1)/2), (0, H/2, 0, (H-1)/2), (0, 0, 0, 1)
            const float hw = pp.width / 2.0f, hwm = (pp.width - 1.0f) / 2.0f, hh = pp.height / 2.0f, hhm = (pp.height - 1.0f) / 2.0f;
            float Tu[3], Tv[3], Tw[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                Tu[r] = X[0][r] * hw + X[3][r] * hwm;
                Tv[r] = X[1][r] * hh + X[3][r] * hhm;
                Tw[r] = X[3][r];
            }
            // :201-221 the three projected points of Tt and the basis vectors, in NDC and in pixels
            float p1[4], p2[4], pc[4];
#pragma unroll
            for (int c = 0; c < 4; c++) { p1[c] = X[c][0] + X[c][2]; p2[c] = X[c][1] + X[c][2]; pc[c] = X[c][2]; }
            const float p1x = p1[0] / p1[3], p1y = p1[1] / p1[3], p2x = p2[0] / p2[3], p2y = p2[1] / p2[3];
            const float pcx = pc[0] / pc[3], pcy = pc[1] / pc[3];
            const float b1x = p1x - pcx, b1y = p1y - pcy, b2x = p2x - pcx, b2y = p2y - pcy;
            const float b1sx = b1x * 0.5f * pp.width, b1sy = b1y * 0.5f * pp.height;
            const float b2sx = b2x * 0.5f * pp.width, b2sy = b2y * 0.5f * pp.height;
            const float len1 = sqrtf(b1sx * b1sx + b1sy * b1sy), len2 = sqrtf(b2sx * b2sx + b2sy * b2sy);
            // the quad: centre and basis in pixels (the viewport transform of ndcCenter.xy + ndcOffset), vQuadCenter
            float B1x, B1y, B2x, B2y, qcx, qcy;
            if (len1 < 1.0f || len2 < 1.0f) {             // minPix = 1: the reference's screen-aligned square (:160-188)
                const float distance = Tw[0] * Tw[0] * 1.0f + Tw[1] * Tw[1] * 1.0f + Tw[2] * Tw[2] * -1.0f;
                const float inv = 1.0f / distance;
                const float f0 = inv * 1.0f, f1 = inv * 1.0f, f2 = inv * -1.0f;
                if (fabsf(distance) < 0.00001f) ok = false;              // the shader returns with gl_Position unwritten
                const float pix = Tu[0] * Tw[0] * f0 + Tu[1] * Tw[1] * f1 + Tu[2] * Tw[2] * f2;
                const float piy = Tv[0] * Tw[0] * f0 + Tv[1] * Tw[1] * f1 + Tv[2] * Tw[2] * f2;
                const float tx = Tu[0] * Tu[0] * f0 + Tu[1] * Tu[1] * f1 + Tu[2] * Tu[2] * f2;
                const float ty = Tv[0] * Tv[0] * f0 + Tv[1] * Tv[1] * f1 + Tv[2] * Tv[2] * f2;
                const float hex = pix * pix - tx, hey = piy * piy - ty;
                const float ex = sqrtf(fmaxf(0.0001f, hex)), ey = sqrtf(fmaxf(0.0001f, hey));
                const float radius = fmaxf(ex, ey);
                const float bvx = 1.0f / pp.width, bvy = 1.0f / pp.height;       // basisViewport
                B1x = radius * 3.0f * bvx * 2.0f * 0.5f * pp.width; B1y = 0.0f;
                B2x = 0.0f; B2y = radius * 3.0f * bvy * 2.0f * 0.5f * pp.height;
                qcx = pix; qcy = piy;
            } else {                                      // the eigen-aligned parallelogram (:227-233)
                B1x = b1x * 3.0f * pp.inv_focal_adj * 0.5f * pp.width; B1y = b1y * 3.0f * pp.inv_focal_adj * 0.5f * pp.height;
                B2x = b2x * 3.0f * pp.inv_focal_adj * 0.5f * pp.width; B2y = b2y * 3.0f * pp.inv_focal_adj * 0.5f * pp.height;
                qcx = pcx; qcy = pcy;                     // center.xy: NDC, as the shader has it
            }
            if (EXT && (pp.flags & GS_CAM_FADE_IN)) {     // SplatMaterial.js:347-363
                const float fx_ = c0 - pp.scene_center[0], fy_ = c1 - pp.scene_center[1], fz_ = c2 - pp.scene_center[2];
                const float center_dist = sqrtf(fx_ * fx_ + fy_ * fy_ + fz_ * fz_);
                float f = center_dist < pp.fade_start ? 0.0f : 1.0f;                   // step(edge, x)
                float t = (center_dist - pp.fade_start) / 0.75f;
                t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                f = (1.0f - f) + (1.0f - t) * f;
                alpha *= 1.0f * f;
            }
            const float cx = (ndcx * 0.5f + 0.5f) * pp.width;
            const float cy = (ndcy * 0.5f + 0.5f) * pp.height;
            if (ok) {
                // pixel bounds of the parallelogram {c + x B1 + y B2 : |x|, |y| <= 1}, a hair wide as k_project's
                const float ext_x = (fabsf(B1x) + fabsf(B2x)) * 1.00001f + 1e-3f;
                const float ext_y = (fabsf(B1y) + fabsf(B2y)) * 1.00001f + 1e-3f;
                float fx0 = ceilf(cx - ext_x - 0.5f), fx1 = floorf(cx + ext_x - 0.5f);
                float fy0 = ceilf(cy - ext_y - 0.5f), fy1 = floorf(cy + ext_y - 0.5f);
                fx0 = fmaxf(fx0, 0.0f); fx1 = fminf(fx1, pp.width - 1.0f);
                fy0 = fmaxf(fy0, 0.0f); fy1 = fminf(fy1, pp.height - 1.0f);
                // (NaN anywhere in the chain fails the comparisons: nothing drawn, as a quad with NaN corners)
                const float det = B1x * B2y - B2x * B1y;
                if (fx0 <= fx1 && fy0 <= fy1 && det == det) {
                    visible = true;
                    const uint32_t tx0 = (uint32_t)fx0 / GS_TILE, tx1 = (uint32_t)fx1 / GS_TILE;
                    const uint32_t ty0 = (uint32_t)fy0 / GS_TILE, ty1 = (uint32_t)fy1 / GS_TILE;
                    rect = make_uint2(tx0 | (ty0 << 16), tx1 | (ty1 << 16));
#pragma unroll
                    for (int r = 0; r < 3; r++) { rec.tu[r] = Tu[r]; rec.tv[r] = Tv[r]; rec.tw[r] = Tw[r]; }
                    rec.qcx = qcx; rec.qcy = qcy;
                    rec.cx = cx; rec.cy = cy;
                    rec.i00 = B2y / det; rec.i01 = -B2x / det;
                    rec.i10 = -B1y / det; rec.i11 = B1x / det;
                    ShPre pre;
                    pre.have = false;
                    sh_colour<EXT>(pp, mp, i, scene, c0, c1, c2, col, pre);
                    rec.c0 = unorm16(col[0]) | (unorm16(col[1]) << 16);
                    rec.c1 = unorm16(col[2]) | (unorm16(alpha) << 16);
                }
            }
        }
    }
    // survivors compacted inside their block, masks and look-up words: k_project's layout (project.hip, project_block), which the
    // binner, the visibility-culled sort and the debug reads consume
    __shared__ uint32_t s_cnt[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long vis = __ballot(visible);
    if (lane == 0u) {
        s_cnt[wave] = (uint32_t)__popcll(vis);
        vis_mask[i >> 6] = vis;
    }
    __syncthreads();
    if (threadIdx.x == 0) block_any[blk] = (s_cnt[0] | s_cnt[1] | s_cnt[2] | s_cnt[3]) ? 1 : 0;
    const uint32_t block_base = blk * 256u;
    uint32_t wave_base = block_base;
#pragma unroll
    for (uint32_t w = 0; w < 3; w++) wave_base += (w < wave) ? s_cnt[w] : 0u;
    if ((lane & 31u) == 0u) {
        const uint32_t lo = (uint32_t)vis, hi = (uint32_t)(vis >> 32);
        vis32[i >> 5] = lane == 0u ? make_uint2(lo, wave_base) : make_uint2(hi, wave_base + (uint32_t)__popc(lo));
    }
    const uint32_t slot = wave_base + (uint32_t)__popcll(vis & ((1ull << lane) - 1ull));
    if (i < pp.count) {
        const BinRect br = {rect.x, rect.y};
        if (NARROW) {
            static_cast<uint32_t*>(prect)[i] = bin_word_pack_narrow(visible, slot - block_base, br);
        } else {
            const BinWordWide w = bin_word_pack_wide(visible, slot - block_base, br);
            static_cast<uint2*>(prect)[i] = make_uint2(w.x, w.y);
        }
    }
    if (visible) {
        recs[slot] = rec;
        rects[slot] = rect;
        if (DEPTH) zrec[slot] = zwin;
        if (vis_orig) {
            const uint32_t orig = inv_perm ? inv_perm[i] : i;
            atomicOr(&vis_orig[orig >> 5], 1u << (orig & 31u));
        }
    }
}

int gs_launch_project_2d(gs_mesh* m, const ProjectParams& pp, const MeshPlanes& mp, ProjSet& ps, uint32_t* vis_orig, const uint32_t* inv_perm,
                         bool block_tested) {
    GS_TRY(ps.recs2d.ensure((size_t)m->max_count * sizeof(SurfelRec)));
    const uint32_t blocks = (pp.count + 255u) / 256u;
    const bool ext = pp.sh_u8 || pp.scene_count > 1 || (pp.flags & (GS_CAM_FADE_IN | GS_CAM_SCENE_EFFECTS | GS_CAM_DYNAMIC));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, m->ctx->aux, pp, mp, ps.recs2d.as<SurfelRec>(), ps.rects.as<uint2>(),
                           ps.vis_mask.as<unsigned long long>(), ps.vis32.as<uint2>(), vis_orig, inv_perm, ps.block_any.as<uint8_t>(),
                           ps.prect.p, ps.zrec.as<float>(), block_tested ? 1u : 0u);
    };
    const bool depth = pp.depth_mode != 0u;
#define GS_PROJECT_2D_LAUNCH(E, D)                                 \
    do {                                                           \
        if (ps.narrow_word) launch(k_project_2d<E, D, true>);      \
        else launch(k_project_2d<E, D, false>);                    \
    } while (0)
    if (ext && depth) GS_PROJECT_2D_LAUNCH(true, true);
    else if (ext) GS_PROJECT_2D_LAUNCH(true, false);
    else if (depth) GS_PROJECT_2D_LAUNCH(false, true);
    else GS_PROJECT_2D_LAUNCH(false, false);
#undef GS_PROJECT_2D_LAUNCH
    return GS_OK;
}
