/*
 * gsplat_hip.h — C ABI of libgsplat_hip.so: the MI355X (gfx950) sort-and-rasterize engine that replaces
 * the two device-facing seams of mkkellogg/GaussianSplats3D.  Plain pointers and sizes only.
 *
 * Every entry point cites the reference interface it replaces (paths relative to /root/reference).
 * The reference has no FFI today; INTEGRATION.md shows the N-API / ctypes bindings a maintainer adds.
 *
 *   SORT SEAM    src/worker/SortWorker.js:202-256 (createSortWorker + message protocol) over the WASM C ABI
 *                src/worker/sorter.cpp:17-22 (sortIndexes)                              -> gs_sorter_*
 *   RENDER SEAM  src/splatmesh/SplatMesh.js (setupDataTextures :637-898, updateRenderIndexes :1228-1235,
 *                updateUniforms :1248-1280) + the GLSL pair SplatMaterial.js:112-341 /
 *                SplatMaterial3D.js:81-255 drawn by renderer.render (src/Viewer.js:1616)  -> gs_mesh_*
 *
 * Threading: calls on one gs_context (and the objects created from it) must be serialised by the caller,
 * like the reference's single sort worker + single GL context.  All device work of a context runs on one
 * HIP stream.  Calls that return data to host memory block until it is there; calls that leave their
 * result on the device only enqueue work.
 *
 * There is NO CPU fallback: every call fails with GS_ERR_HIP if no gfx950 device is usable.
 */
#ifndef GSPLAT_HIP_H
#define GSPLAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 5   /* 5: + gs_mesh_set_draw_mode (round 6); 4: + gs_mesh_set_destination (round 5); earlier entry points unchanged */

/* status codes (negative = error, positive = warning, result still defined) */
#define GS_OK 0
#define GS_WARN_KEY_CLAMPED 1   /* a depth bucket fell outside [0,range): the reference corrupts memory here  */
#define GS_WARN_FRAME_TRUNCATED 2 /* gs_mesh_render: an EARLIER asynchronous draw overflowed its entry buffer (its frame
                                     lacks the farthest entries of some lists); the buffers have been grown, this draw and
                                     the following ones are complete                                                   */
#define GS_ERR_INVALID (-1)     /* bad argument                                                               */
#define GS_ERR_HIP (-2)         /* HIP runtime / device failure (see gs_last_error)                            */
#define GS_ERR_NOMEM (-3)
#define GS_ERR_CAPACITY (-4)    /* tile-entry buffer overflow even after growing to the configured limit       */
#define GS_ERR_UNSUPPORTED (-5)

typedef struct gs_context gs_context;
typedef struct gs_sorter gs_sorter;
typedef struct gs_mesh gs_mesh;
typedef struct gs_tree gs_tree;

/* Message of the last failing call on this thread (the reference throws JS Errors, SplatMesh.js:1518-1533). */
const char* gs_last_error(void);
int gs_abi_version(void);
/* Number of visible HIP devices, or a negative status. */
int gs_device_count(void);

/* One context per GPU.  hip_stream: an existing hipStream_t to enqueue on (e.g. PyTorch's current
 * stream) or NULL to let the library create its own. */
int gs_context_create(int device, void* hip_stream, gs_context** out);
/* The same with explicit flags.  GS_CTX_SINGLE_STREAM: sorts, the vertex stage and the rest of a draw all run on the one
 * stream (no worker / aux streams), i.e. a frame is strictly sort -> draw.  gs_context_create takes this flag from the
 * environment (GSPLAT_SERIAL=1); the default is the reference's shape: the sort runs concurrently with drawing, like its
 * Web Worker (src/worker/SortWorker.js). */
#define GS_CTX_SINGLE_STREAM 1u
#define GS_CTX_STAGE_TIMING 2u /* bracket the stages of EVERY sort / draw with timing events, so that gs_sorter_last_stats /
                                  gs_mesh_last_stats can time calls that were made without a stats pointer.  By default only
                                  calls that pass `stats` (and therefore synchronise anyway) are timed and the *_ms fields
                                  read 0 after any other call: an event record is a barrier packet on the stream, nine of them
                                  per frame cost 35 us of a 0.33 ms frame on MI355X */
#define GS_CTX_FORK_JOIN 4u    /* multi-stream context whose FRAMES stay serial: the sort and the vertex stage of a frame run side by
                                  side on their own streams (they share nothing: the sort reads the centres, the vertex stage
                                  the mesh planes) and join where the binner needs both, but no sort starts before everything the
                                  context's stream held when it was called has finished - frame k + 1 never overlaps frame k.
                                  The default context lets the next sort overlap the tail of the previous draw (throughput);
                                  this one shortens the frame itself: t_frame = max(t_sort, t_vertex) + t_bin + t_blend */
int gs_context_create_ex(int device, void* hip_stream, uint32_t flags, gs_context** out);
void gs_context_destroy(gs_context* ctx);
int gs_context_synchronize(gs_context* ctx);
/* Turn GS_CTX_STAGE_TIMING on (enable != 0) or off for the sorts / draws that follow (e.g. while a profiling overlay is up). */
int gs_context_set_stage_timing(gs_context* ctx, int enable);

/* ------------------------------------------------------------------------------------------------ *
 * SORT SEAM
 * ------------------------------------------------------------------------------------------------ */
#define GS_SORT_INTEGER 1u  /* integerBasedSort (Viewer option, src/Viewer.js:95-98): int32 centres x1000      */
#define GS_SORT_DYNAMIC 2u  /* dynamicMode: per-splat scene index + per-scene transform (sorter.cpp:41-62)     */
#define GS_MAX_SCENES 32u   /* src/Constants.js:7 */

/* createSortWorker(splatCount, useSharedMemory, enableSIMDInSort, integerBasedSort, dynamicMode,
 * splatSortDistanceMapPrecision) — src/worker/SortWorker.js:202-256.  Shared-memory / SIMD flavours of
 * the WASM module have no meaning here.  precision_bits: 10..20 (integer) / 10..24 (float),
 * src/Viewer.js:208-210. */
int gs_sorter_create(gs_context* ctx, uint32_t max_splat_count, uint32_t flags, uint32_t precision_bits,
                     gs_sorter** out);
void gs_sorter_destroy(gs_sorter* s);

/* The {centers, sceneIndexes, range:{from,count}} message — src/worker/SortWorker.js:84-98.
 * centers_aos4: int32[4*count] (GS_SORT_INTEGER; SplatMesh.getIntegerCenters(padFour), SplatMesh.js:1912-1926)
 * or float[4*count].  scene_indexes: uint32[count], required iff GS_SORT_DYNAMIC. */
int gs_sorter_upload_centers(gs_sorter* s, uint32_t from, uint32_t count, const void* centers_aos4,
                             const uint32_t* scene_indexes);

typedef struct gs_sort_stats {
    float device_ms;        /* sortTime of the sortDone message (SortWorker.js:76-78), device clock; 0 if the
                               sort was made without `stats` and without GS_CTX_STAGE_TIMING                 */
    int32_t key_min;        /* minDistance / maxDistance of sorter.cpp:24-25,72-73                           */
    int32_t key_max;
    uint32_t clamped;       /* buckets forced into [0,range)                                                  */
    uint32_t passes;        /* 8-bit LSD radix passes used                                                    */
    uint32_t result_count;  /* length of the sorted result: splatRenderCount, or the kept count under
                               gs_sorter_set_frustum_cull                                                     */
} gs_sort_stats;

/* The {sort:{modelViewProj, splatRenderCount, splatSortCount, usePrecomputedDistances, indexesToSort,
 * transforms, precomputedDistances}} message -> sortIndexes (sorter.cpp:17-22) -> {sortDone, sortedIndexes}.
 *   mvp              float[16] column-major (fp32 as written into WASM memory, SortWorker.js:54)
 *   indexes_to_sort  uint32[render_count] host, or NULL = identity list (Viewer.js:2061-2073)
 *   precomputed      int32/float[splat_count] host or NULL (usePrecomputedDistances)
 *   transforms       float[16*GS_MAX_SCENES] host, required iff GS_SORT_DYNAMIC
 *   sorted_out       uint32[render_count] host or NULL (result stays on the device for gs_mesh_render)
 * Result: [0, render-sort) copied; tail = far->near buckets, ties in reverse input order. */
int gs_sorter_sort(gs_sorter* s, const float* mvp, const uint32_t* indexes_to_sort, uint32_t sort_count,
                   uint32_t render_count, const void* precomputed, const float* transforms,
                   uint32_t* sorted_out, gs_sort_stats* stats);

/* The same sort, fed by the device-resident indexesToSort list (and splatRenderCount) that the last
 * gs_tree_gather(tree, ..., s, ...) left in this sorter: no index list crosses PCIe. */
int gs_sorter_sort_gathered(gs_sorter* s, const float* mvp, uint32_t sort_count, const void* precomputed,
                            const float* transforms, uint32_t* sorted_out, gs_sort_stats* stats);

/* uploadedSplatCount without centres: a Viewer with gpuAcceleratedSort never posts the `centers` message (src/Viewer.js:1124-1136)
 * and sorts only precomputed distances.  Raises the sorter's uploaded splat count to `count` (<= max_splat_count); splats
 * that never received centres get zero ones, what the reference's zero-filled WASM memory holds.  A smaller count is a no-op. */
int gs_sorter_set_uploaded_count(gs_sorter* s, uint32_t count);

/* Remove centres on the device (Viewer.removeSplatScenes without rebuilding the worker, src/Viewer.js:1326-1429): the sorter's half
 * of gs_mesh_remove, same arguments and renumbering.  A sorter accepts any ranges.  Afterwards every sort's list is what a fresh
 * sorter of the same capacity and flags gives that received the surviving centres at their new positions: the SoA planes, the
 * extreme set and the 16-bit centre planes are derived again from the surviving rows.  The call waits for the sort in flight; the
 * resident result, a gathered list, the per-tree caches and device distances are dropped - sort again (and gather from a new
 * tree) before the next draw.  GS_ERR_INVALID, and nothing changes, on malformed ranges. */
int gs_sorter_remove(gs_sorter* s, const uint32_t* ranges, uint32_t n_ranges, const uint32_t* scene_remap,
                     uint32_t scene_remap_count);

/* Change the capacity of a live sorter on the device: the sorter's half of gs_mesh_resize (a Viewer whose maxSplatCount changed
 * drops its sort worker and sends every centre again, src/Viewer.js:1123-1136).  uploaded splat count <= max_splat_count, larger
 * or smaller than the current capacity.  Afterwards every sort's list is what a fresh sorter of the new capacity and the same flags
 * gives that received the same centres by the same uploads: the rows as uploaded, the SoA planes and the scene indexes are copied
 * on the device, the 16-bit centre planes are derived again, the extreme set stays (it depends on the rows alone), and the
 * key / value / result buffers are allocated again as gs_sorter_create (or their first user) allocates them.  Flags, precision,
 * cull switches and the mesh binding stay.  The call waits for the sort in flight; the resident result, a gathered list, the
 * per-tree caches and device distances are dropped - sort again before the next draw.
 * GS_OK and nothing happens when max_splat_count is the current capacity.  GS_ERR_INVALID, and nothing changes, for 0 or a value
 * below the uploaded splat count.  GS_ERR_NOMEM: as for gs_mesh_resize - what the call allocated is released before the key /
 * value buffers come back at their old size, the sorter keeps its capacity and its centres and stays usable; should even that
 * fail, sorts are refused (GS_ERR_INVALID) until a gs_sorter_resize succeeds. */
int gs_sorter_resize(gs_sorter* s, uint32_t max_splat_count);

/* Optional coupling of the two seams: a sorter bound to a mesh leaves its device-resident result as positions in
 * that mesh's internal storage order, so gs_mesh_render(m, ..., sorter = s, ...) needs no per-frame index translation.
 * Host-visible results (sorted_out, gs_sorter_debug_read) are always the caller's splat indexes.  m = NULL unbinds. */
int gs_sorter_bind_mesh(gs_sorter* s, gs_mesh* m);

/* Per-splat frustum cull fused into the sort (no counterpart in the reference, whose cull works on octree nodes,
 * src/Viewer.js:1969-2077; composes with gs_tree_gather).  With enable != 0 a full sort (sort_count == render_count,
 * static scene, no precomputed distances) keeps only the list positions whose centre passes
 *     q = mvp * (x, y, z, 1) in fp32;  |q.x| <= 1.25 q.w + 0.01,  |q.y| <= 1.25 q.w + 0.01,  |q.z| <= 1.01 q.w + 0.01
 * which for the same camera is a superset of what the vertex stage can draw (it drops at 1.2 w, SplatMaterial.js:160-164).
 * Keys, min / max and buckets are still taken over every list position, so the result is exactly the reference's sorted
 * list with the dropped splats removed and a frame drawn from it is bit-identical to one drawn from the full list.
 * The result's length lives on the device (gs_sort_stats.result_count after a sync); gs_mesh_render reads it there:
 * pass the sort's render_count as usual. */
int gs_sorter_set_frustum_cull(gs_sorter* s, int enable);

/* Visibility cull: the exact version of the above, for a sorter bound to a mesh (gs_sorter_bind_mesh).  After
 * gs_mesh_project(m, cam) a full sort keeps exactly the list positions whose splat survived the mesh's vertex stage for
 * `cam` - every reject of the shaders (SplatMaterial.js:160-164, SplatMaterial3D.js:188), an empty pixel footprint, and the
 * camera's strip of tile rows (gs_camera.tile_row_begin / end).  Keys, min / max and buckets are still taken over every
 * list position, so the result is the reference's sorted list restricted to the splats this frame (this rank's strip)
 * draws, and the frame is bit-identical.  This is how the tile-row strips of a multi-GPU draw shard the sort: each rank
 * keys all splats (12 bytes each) but radix-sorts and bins only its own.  Order per frame:
 *     gs_mesh_project(m, cam) -> gs_sorter_sort(s, mvp of the same camera, ...) -> gs_mesh_render(m, cam, sorter = s).
 * A GS_SORT_DYNAMIC sorter culls the same way (20 bytes per splat keyed: x, y, z, w and the scene index): the sort takes
 * `transforms` as any dynamic sort does, and the mesh's projection must have been made with GS_CAM_DYNAMIC and the same scene
 * transforms (gs_mesh_set_scenes) - the mask is what THAT projection drew.  A scene index >= GS_MAX_SCENES gives an unspecified key.
 * Refused (GS_ERR_INVALID at the sort): a partial sort (sort_count < render_count) and precomputed distances under the cull, for
 * either kind of sorter; for a dynamic one also a gathered list whose length lives on the device (gs_tree_gather with
 * render_count == NULL).  gs_sorter_set_frustum_cull keeps refusing a dynamic sorter. */
int gs_sorter_set_visibility_cull(gs_sorter* s, int enable);

/* Test hooks: intermediates of the last sort, positions [0, render_count) (valid in the sorted tail).
 * what: 0 = int32 depth keys (mappedDistances before mapping), 1 = int32 buckets (after), 2 = sorted,
 *       3 = keep bits of the last culled sort, bit (i & 31) of uint32 word i >> 5: per list position i after a frustum-culled
 *           sort, per ORIGINAL splat index i (the bound mesh's visibility mask as the sort consumed it) after a
 *           visibility-culled one,
 *       4 = the last sort's front end, up to 8 host words: {1 = the known-range kernel ran, size of the extreme set of the
 *           centres (0: none), lo, hi of the key range as the host computed it (0, 0 on the other path), 1 = the set covers
 *           the current centres, pass 0's slot of group rows, 1 = the sort stored 16-bit radix keys instead of the depths,
 *           1 = that kernel read the centres as 16-bit offset planes (an extreme set no wider than 65535 per axis; off with
 *           $GSPLAT_NO_COMPACT_CENTRES) instead of the int32 planes},
 *       5 = the last sort's host plan, host words: the inputs it was planned from, then the plan that ran - every field a
 *           32-bit word, in the order of SortPlanIn and SortPlan in csrc/sort_plan.hpp (typed by tests/sort_plan_cases.py): the
 *           front end and its grids, what became of a pending gather, pass 0's slot, and per radix pass its loader, output,
 *           shifts, slot and grid.
 * Selectors 0 and 1 always describe the sort that ran.  A sort that stored 16-bit radix keys (word 6 of selector 4) keeps
 * no depths: they are rebuilt on the device from the centres and that sort's coefficients when a selector asks for them,
 * and before an upload of centres overwrites what they are made from. */
int gs_sorter_debug_read(gs_sorter* s, int what, void* dst, uint32_t count);

/* ------------------------------------------------------------------------------------------------ *
 * CULL (feeds the sort seam): the reference's octree and its per-sort frustum cull
 * ------------------------------------------------------------------------------------------------ */
/* SplatMesh.buildSplatTree -> SplatTree.processSplatMesh -> worker createSplatTree
 * (src/splatmesh/SplatMesh.js:231-280, src/splattree/SplatTree.js:132-271, 320-420).
 *   centers      float[3*count], SplatMesh.getSplatCenter of splats first_index .. first_index+count-1
 *   keep         uint8[count] or NULL: the alpha filter `splatColor.w >= minAlpha` (SplatMesh.js:239-244)
 *   max_depth / max_centers_per_node   8 / 1000 in the reference (SplatMesh.js:236)
 * The tree is built on the host with the reference's arithmetic (leaves, their order and their index lists are
 * identical); with ctx != NULL it is mirrored to the device for gs_tree_gather, with ctx == NULL it is host-only. */
int gs_tree_create(gs_context* ctx, const float* centers, const uint8_t* keep, uint32_t count, uint32_t first_index,
                   uint32_t max_depth, uint32_t max_centers_per_node, gs_tree** out);
void gs_tree_destroy(gs_tree* t);

typedef struct gs_tree_info {
    uint32_t leaves;        /* subTree.nodesWithIndexes.length (leaves holding >= 1 index)                    */
    uint32_t all_leaves;    /* countLeaves()                                                                  */
    uint32_t nodes;
    uint32_t splats;        /* sum of the leaves' index counts                                                */
    double scene_min[3], scene_max[3];
} gs_tree_info;
int gs_tree_get_info(gs_tree* t, gs_tree_info* info);
/* Leaves in nodesWithIndexes (depth-first) order; any pointer may be NULL.  bounds double[6*leaves] = min xyz,
 * max xyz; centers double[3*leaves]; depths uint32[leaves]; offsets uint32[leaves+1]; indexes uint32[splats]. */
int gs_tree_read(gs_tree* t, double* bounds, double* centers, uint32_t* depths, uint32_t* offsets, uint32_t* indexes);

/* Viewer.gatherSceneNodesForSort (src/Viewer.js:1969-2077). */
typedef struct gs_gather_params {
    double model_view[16];   /* inverse(camera.matrixWorld) * splatMesh.matrixWorld, fp64, column-major (:1999-2000) */
    double fov_y_deg;        /* camera.fov                                                                    */
    double render_width, render_height;   /* getRenderDimensions                                              */
    uint32_t gather_all;     /* gatherAllNodes                                                                */
    uint32_t pad;
} gs_gather_params;
/* Tests every leaf, orders the kept ones by distance and lays their index lists out far -> near (the nearest leaf
 * ends the buffer), on the device: four small launches plan where every kept leaf's list goes (a count-weighted rank by
 * distance), then the lists are copied - at once, or, when a static sorter is the only reader, by that sorter's next full sort,
 * fused with its key kernel (the list is then in place when gs_sorter_sort_gathered returns).
 *   dst               sorter whose device-side indexesToSort buffer receives the list (then call
 *                     gs_sorter_sort_gathered), or NULL
 *   render_count      out: splatRenderCount (this waits for the device); or NULL = asynchronous: nothing returns to the host,
 *                     the count stays on the device next to the list (needs dst, no host copy).  A following
 *                     gs_sorter_sort_gathered(dst, ..., sort_count >= the tree's splat count) then sorts the whole list
 *                     without ever learning its length on the host, and gs_mesh_render(..., sorter = dst, render_count =
 *                     the tree's splat count) draws it: the frame needs no host round trip at all
 *   indexes_out_host  uint32[tree splats] host copy of the list, or NULL */
int gs_tree_gather(gs_tree* t, const gs_gather_params* params, gs_sorter* dst, uint32_t* render_count,
                   uint32_t* indexes_out_host);

/* The octree of a dynamicMode mesh: SplatTree.processSplatMesh builds ONE SUB-TREE PER SCENE over that scene's untransformed
 * centres (src/splattree/SplatTree.js:378-390, worker :252-271), and Viewer.gatherSceneNodesForSort tests each sub-tree's
 * leaves under its own scene's transform and pools the kept leaves of all of them into one list (src/Viewer.js:1999-2055).
 *   centers / keep       the scenes back to back: scene s owns the global indexes sum(counts[<s]) .. sum(counts[<=s]) - 1
 *   scene_count          1 .. GS_MAX_SCENES; 1 is gs_tree_create(ctx, centers, keep, counts[0], 0, ...), leaf for leaf
 *   scene_splat_counts   uint32[scene_count]
 * Every sub-tree is built as gs_tree_create builds a tree over the scene's range with first_index = the range's start (its
 * own root box, the same build).  gs_tree_read returns the sub-trees' nodesWithIndexes one after the other, in scene order;
 * gs_tree_get_info sums the counts and reports the union of the scenes' boxes.  A scene whose filter keeps nothing has no leaf. */
int gs_tree_create_scenes(gs_context* ctx, const float* centers, const uint8_t* keep, uint32_t scene_count,
                          const uint32_t* scene_splat_counts, uint32_t max_depth, uint32_t max_centers_per_node, gs_tree** out);
/* first_leaf uint32[scene_count + 1]: where each sub-tree starts in what gs_tree_read returns ({0, leaves} for a tree from
 * gs_tree_create). */
int gs_tree_scene_leaves(gs_tree* t, uint32_t* first_leaf);
/* gs_tree_gather with one modelView per scene; dst / render_count / indexes_out_host as there (synchronous and asynchronous
 * forms, host copy, sorter hand-over).
 *   params->model_view   the BASE matrix.  In dynamic mode the reference does NOT multiply splatMesh.matrixWorld into it
 *                        (src/Viewer.js:2000): pass inverse(camera.matrixWorld) alone
 *   scene_transforms     double[16 * transform_count], column-major, SplatMesh.getSceneTransform(s); scene s is tested under
 *                        base x transform_s (Matrix4.multiplyMatrices' expression order, fp64, unfused).  NULL: every scene is
 *                        tested under the base (transform_count is then ignored)
 *   transform_count      must equal the tree's scene count, else GS_ERR_INVALID
 * Leaves at the same distance keep the order in which the reference appends them: sub-tree first, nodesWithIndexes second.
 * A tree of several sub-trees never defers its copy to the sorter.  gs_tree_gather on such a tree is this call with NULL. */
int gs_tree_gather_scenes(gs_tree* t, const gs_gather_params* params, const double* scene_transforms, uint32_t transform_count,
                          gs_sorter* dst, uint32_t* render_count, uint32_t* indexes_out_host);

/* ------------------------------------------------------------------------------------------------ *
 * ASSETS (host side, no GPU needed): the reference's file readers up to the arrays the seams consume
 * ------------------------------------------------------------------------------------------------ */
typedef struct gs_asset gs_asset;
#define GS_ASSET_PLY 1u      /* .ply, binary little endian; the flavour is decided from the header as PlyParserUtils.js:257-271
                              * does: `element chunk` / `packed_` = PlayCanvas (SuperSplat) compressed
                              * (src/loaders/ply/PlayCanvasCompressedPlyParser.js), `element codebook_centers` = INRIA-v2
                              * (src/loaders/ply/INRIAV2PlyParser.js: half-float centres, one uchar index per attribute into
                              * 256-entry codebook pages; kept in FILE order, every splat, as .splat is - the reference's array
                              * path drops and reorders), anything else INRIA-v1 (src/loaders/ply/INRIAV1PlyParser.js).
                              * An INRIA-v2 file is refused by name (`INRIA-v2 PLY: ...`) for: a format other than
                              * binary_little_endian, no end_header, an unsized property type, an element count that is no
                              * number below 2^32, more than one element besides codebook_centers or none, x / y / z or
                              * rot_0..3 missing, x / y / z not short / ushort, an index field not uchar, an f_rest count outside
                              * 0 / 9 / 24 / 45, a codebook property that is read and is not short / ushort, fewer than 256
                              * codebook rows, a codebook page the file's fields need missing, element data beyond the end of
                              * the file, a row of 64 KiB or more.  A degree-3 file is read at degree 2                    */
#define GS_ASSET_KSPLAT 2u   /* .ksplat, compression levels 0/1/2: src/loaders/SplatBuffer.js                        */
#define GS_ASSET_SPLAT 3u    /* .splat, 32-byte rows (centre 3 x f32, scale 3 x f32, RGBA, rotation 4 x u8), SH degree 0:
                              * src/loaders/splat/SplatParser.js:13-56, the progressive file-order path - every splat is
                              * kept and alpha is only zeroed at fill time by min_alpha (the array path of SplatLoader.js:12-22
                              * drops and reorders splats; that is not this interface's "file order")                 */
enum { GS_ASSET_SPZ = 4 };   /* .spz, versions 1 and 2: a gzip member around a 16-byte header and six byte planes (positions,
                              * alphas, colours, scales, rotations, SH): src/loaders/spz/SpzLoader.js with optimizeSplatData
                              * false.  Inflated by the library's own reader (no zlib); refused by name: a damaged gzip (CRC-32,
                              * ISIZE, truncation, bytes behind the trailer), a wrong magic, a version outside 1..2, more than
                              * 10 000 000 points, an SH degree above 3, a stream that is not exactly header + planes.  A
                              * degree-3 file is read at degree 2.  An enum constant, unlike its siblings: same value space   */
/* Parses `data` (the bytes of the file).  max_sh_degree: outSphericalHarmonicsDegree (Viewer option
 * sphericalHarmonicsDegree); splats keep FILE order (the reference's optimizeSplatData:false).  A .splat / compressed
 * PLY / INRIA-v2 PLY / .spz asset keeps the file's own rows (.spz: the inflated planes; INRIA-v2: with the codebook decoded once,
 * at open): gs_mesh_upload_asset /
 * gs_sorter_upload_asset_centers send those to the device and decode them there, gs_asset_fill decodes them on the host the first time it is called (compression_level 0, sh_level 1). */
int gs_asset_open(const void* data, uint64_t bytes, uint32_t format, uint32_t max_sh_degree, gs_asset** out);
void gs_asset_close(gs_asset* a);
typedef struct gs_asset_info {
    uint32_t splat_count;
    uint32_t sh_degree;          /* degree the fill arrays carry                                                */
    uint32_t compression_level;  /* of the splat buffer: 0 (also every PLY), 1, 2                                */
    uint32_t sh_level;           /* getTargetSphericalHarmonicsCompressionLevel: 1 = fp16 output, 2 = uint8      */
    float scene_center[3];
    float sh_min, sh_max;        /* min/maxSphericalHarmonicsCoeff of the file (8-bit SH range)                  */
} gs_asset_info;
int gs_asset_get_info(gs_asset* a, gs_asset_info* info);
/* The scene transform SplatMesh.fillSplatDataArrays hands to the SplatBuffer fills in static mode
 * (SplatMesh.js:1872-1899, getSceneTransform :2019-2028): 16 doubles, column-major, THREE.Matrix4.elements.
 * NULL removes it (the reference's `transform === undefined` path, the state of a freshly opened asset).  An identity
 * matrix is NOT the same as NULL for SH: with a matrix the coefficients are widened, rotated in double and converted
 * from level 0 again (SplatBuffer.js:663-673, 684-688), which moves uint8 values of a level-2 file.  From then on
 * gs_asset_fill, gs_mesh_upload_asset and gs_sorter_upload_asset_centers return what the reference returns with that
 * `transform` argument: centres through Vector3.applyMatrix4 (SplatBuffer.js:340-342), covariances as T3 C T3^T
 * (:461-466), SH bands 1 and 2 rotated by the matrix's rotation (:628-637, 766-817); rgba is unaffected.  Replaces
 * the `transform` parameter of SplatBuffer.fillSplatCenterArray / fillSplatCovarianceArray /
 * fillSphericalHarmonicsArray and the decompose + band rows fillSphericalHarmonicsArray derives per call.
 * GS_ERR_INVALID, and the asset keeps the transform it had, for a non-finite element, a bottom row other than
 * (0, 0, 0, 1) (Matrix4.compose never makes another) or a basis column of length 0 (Matrix4.decompose divides by it). */
int gs_asset_set_transform(gs_asset* a, const double* transform16);
/* SplatMesh.fillSplatDataArrays (src/splatmesh/SplatMesh.js:1853-1902), with the scene transform of
 * gs_asset_set_transform if one is set (static mode) and without one otherwise (dynamic mode); any pointer may
 * be NULL.  centers float[3n]; cov_f32 float[6n] / cov_f16 half bits[6n] (covariance compression level 0 / 1);
 * rgba uint8[4n] with alpha zeroed below min_alpha; sh_f16 half bits[ncoef*n] (sh_level 1) or sh_u8 uint8[ncoef*n]
 * (sh_level 2), coefficient-major RGB triples; scales float[3n], rotations float[4n] (x,y,z,w) normalised with
 * w >= 0, as fillSplatScaleRotationArray returns them (SplatBuffer.js:349-437) - untransformed only: asking for them
 * while a transform is set is GS_ERR_INVALID (the transformed fillSplatScaleRotationArray serves the raycaster and
 * 2D mode). */
int gs_asset_fill(gs_asset* a, uint32_t min_alpha, float* centers, float* cov_f32, uint16_t* cov_f16, uint8_t* rgba,
                  uint16_t* sh_f16, uint8_t* sh_u8, float* scales, float* rotations);

/* STREAMED ASSETS: a file handed over as it arrives (the reference's progressive loading: PlyLoader / SplatLoader / KSplatLoader
 * build the scene section by section while the file downloads).  gs_asset_open_stream opens an asset without bytes,
 * gs_asset_append hands it the next piece, and after every append gs_mesh_upload_asset / gs_sorter_upload_asset_centers take
 * any range of the splats that are ready - the file's rows cross to the device and are decoded there, as for an opened asset.
 *   M (whole file)  once the final append is accepted the stream IS the asset gs_asset_open returns for the concatenated bytes,
 *                   in gs_asset_get_info, gs_asset_fill, gs_asset_set_transform, gs_mesh_upload_asset,
 *                   gs_sorter_upload_asset_centers and gs_asset_encode_ksplat.  Where gs_asset_open would refuse the
 *                   concatenation, the append that makes that certain is refused with gs_asset_open's message: a header fault at
 *                   the append that completes the header; "data exceeds the file" and the .spz container checks at `final`.
 *                   (A file with two faults: the stream names the one that is certain first - it cannot know where the file ends
 *                   before `final` - where gs_asset_open names the one it meets first.)
 *                   One exception: a streamed INRIA-v1 PLY keeps the file's own rows and decodes them with the e^x of the
 *                   other row formats (the fdlibm text JavaScript engines run) where gs_asset_open calls the C library's; after
 *                   the fp32 store of a scale and the floor(. * 255) of an opacity the two agree except on rare boundary inputs.
 *                   A NaN its quaternion arithmetic generates is stored as the canonical quiet NaN.  A row of 64 KiB or more is
 *                   refused.
 *   P (prefix)      at any moment the ready splats are a prefix [0, splats_ready) of the whole file's numbering; splats_ready
 *                   never decreases; an upload of a range inside the prefix leaves what the same call on the whole-file asset
 *                   leaves; a range beyond it is GS_ERR_INVALID and nothing changes.
 * A splat is ready when every byte its decode reads has arrived:
 *   INRIA-v1 PLY    row by row behind the header (which may arrive split anywhere); no end_header within the first 1 MiB: refused
 *   compressed PLY  nothing until the chunk element is complete, then vertex row by vertex row; with an output SH degree above 0
 *                   a splat also needs its SH row, in practice the end of the file - open at degree 0 for early splats
 *                   (the reference's own rule, PlyLoader.js:120-125)
 *   .splat          floor(received / 32); expected_bytes is required (the splat count comes from it: the reference needs the
 *                   content length) and bytes beyond it are refused
 *   .ksplat         nothing until the header and every section header are in; a section's rows row by row once its bucket
 *                   block (partial lengths and centres) has arrived and passed the table checks; sections in file order
 *   .spz, INRIA-v2  0 until the final append, then all (a gzip member ends in its CRC; the codebook may follow the rows)
 * expected_bytes (0 = not known) is reserved up front; the stream keeps one copy of the bytes.  Until the stream is complete
 * gs_asset_fill and gs_asset_encode_ksplat are GS_ERR_INVALID, and gs_asset_get_info is until header_ready.  A refused append
 * consumes nothing and sets `failed`: the ready rows stay uploadable, every later append is refused.  An empty append is fine; an
 * append after `complete` is refused.  NO LOCK: the appends and uploads of one asset come from one thread, or the caller
 * serialises them. */
int gs_asset_open_stream(uint32_t format, uint32_t max_sh_degree, uint64_t expected_bytes, gs_asset** out);
int gs_asset_append(gs_asset* a, const void* data, uint64_t bytes, int final);
typedef struct gs_asset_stream_info {
    uint64_t bytes_received;
    uint32_t header_ready;   /* gs_asset_get_info answers (splat_count, sh_degree, levels, ...) */
    uint32_t splats_ready;   /* the rows [0, splats_ready) can be uploaded now */
    uint32_t complete;       /* the final append was accepted */
    uint32_t failed;         /* an append was refused: no further append is taken */
} gs_asset_stream_info;
int gs_asset_get_stream_info(gs_asset* a, gs_asset_stream_info* info);

/* The reference's offline conversion (util/create-ksplat.js, KSplatLoader.downloadFile) on the device: an opened asset ->
 * a one-section .ksplat at compression level 0, 1 or 2.  The file is byte for byte what
 * SplatBuffer.generateFromUncompressedSplatArrays([rows], min_alpha, compression_level, scene_center, block_size,
 * bucket_size) returns (src/loaders/SplatBuffer.js:1177-1326), `rows` holding the values of the source's LEVEL-0 ROWS in file
 * order: three fp32 centres, three fp32 scales, the four rotation floats in slot order, the colour bytes and the fp32 SH of
 * the opened degree.  One section, file order, no SplatPartitioner (its sort's tie order is the engine's, not the format's).
 *   dropped          alpha < min_alpha (:1219); the kept splats keep file order
 *   SH range         scanned over ALL rows, dropped ones too, components FRC0..FRC22 only (:1193: the 24th never takes part),
 *                    by `!m || v < m` (:1194-1199: a running 0 or NaN is replaced by whatever comes next), `|| -1.5` / `|| 1.5`
 *                    at the end (:1204-1205); written into the header at every level, used by toUint8 at level 2
 *   bucket ids       computeBucketsForUncompressedSplatArray (:1328-1399): exact min / max of the kept centres, y/zBlocks =
 *                    ceil(dim / block_size), xBlock = floor((c - min) / block_size) as an IEEE fp64 subtraction and division,
 *                    id = xBlock * (yBlocks * zBlocks) + yBlock * zBlocks + zBlock; a centre on the far face shares an id
 *   buckets          a bucket's centre is the block centre of the splat that opened it (:1365-1375); it closes at bucket_size
 *                    splats and the id opens a new one (:1379-1382); full buckets in closing order, then the open ones in
 *                    ascending id order (:1386); rows are written bucket by bucket at level 0 too (:1245-1257)
 *   rows             writeSplatDataToSectionBuffer (:1075-1173): the quaternion normalised again in double, `|| 0` on scale
 *                    and SH, level-1/2 centres clamp(Math.round(delta * (32767 / (block_size * 0.5))) + 32767, 0, 65535)
 *                    against the double bucket centre, halves by THREE.DataUtils.toHalfFloat, level-2 SH by toUint8
 *   headers          writeHeaderToBuffer (:856-875), writeSectionHeaderToBuffer (:944-960): a level-0 section header carries 0
 *                    for bucket size, bucket count, block size and scale range
 * Only the source's file rows cross to the device; the bucket bookkeeping runs there as a stable sort by id.
 * Refused with nothing produced, the parameter checks before the device is touched: GS_ERR_INVALID for a level outside 0..2,
 * unknown flags, a block_size that is negative or not finite, a bucket_size above 65535 (0 selects the reference's default in
 * both, as its `||` does), a source with a scene transform, no splat surviving min_alpha, a kept centre that is not finite (its
 * id would be the property name "NaN"); GS_ERR_UNSUPPORTED for a source of compression_level 1 or 2 (its values are
 * quantised already) and for a scene of 2^32 - 1 or more blocks (JavaScript's key order stops being numeric there). */
typedef struct gs_ksplat_params {
    uint32_t compression_level;   /* 0, 1, 2                                                                      */
    uint32_t min_alpha;           /* alphaRemovalThreshold                                                        */
    uint32_t bucket_size;         /* 0 = 256 (SplatBuffer.BucketSize)                                             */
    float    block_size;          /* 0 = 5.0 (SplatBuffer.BucketBlockSize)                                        */
    float    scene_center[3];
    uint32_t flags;               /* 0                                                                            */
} gs_ksplat_params;
/* out: a new GS_ASSET_KSPLAT asset that owns the encoded bytes, exactly as gs_asset_open of those bytes would be (close it
 * with gs_asset_close); order_out_host: uint32 per kept splat, the source index stored at each output position, or NULL */
int gs_asset_encode_ksplat(gs_context* ctx, gs_asset* src, const gs_ksplat_params* p, gs_asset** out, uint32_t* order_out_host);
/* The file image of an encoder result (valid until gs_asset_close); GS_ERR_INVALID for other assets */
int gs_asset_bytes(gs_asset* a, const void** data, uint64_t* bytes);

/* ------------------------------------------------------------------------------------------------ *
 * RENDER SEAM
 * ------------------------------------------------------------------------------------------------ */
#define GS_MESH_COV_HALF 1u   /* halfPrecisionCovariancesOnGPU (SplatMesh.js:667-670,735-739)                 */
#define GS_MESH_KEEP_ORDER 4u /* keep splats in upload order on the device (default: each upload is re-ordered along a
                                 Morton curve internally; indexes at this ABI are always the caller's)            */
#define GS_MESH_SH_U8 2u      /* SH stored as uint8 (compression level 2, SplatMesh.js:680-684,789,1064-1066):
                                 sphericalHarmonics8BitMode, dequantised per scene as v/255*(max-min)+min      */
#define GS_SH_F16 0u          /* SH as fp16 (compression level <= 1, SplatMesh.js:1064-1066)                  */
#define GS_MESH_SURFEL 8u     /* splatRenderMode: SplatRenderMode.TwoD (2D Gaussian splatting; SplatMesh.js:666-675, 763-786,
                                 SplatMaterial2D.js): per splat the mesh stores scale x, y, z and rotation x, y, z (w is rebuilt in
                                 the vertex stage) where a 3D mesh stores the six covariance values, always in fp32 - with
                                 GS_MESH_COV_HALF gs_mesh_create is GS_ERR_INVALID (the reference keeps
                                 scaleRotationCompressionLevel 0 whatever halfPrecisionCovariancesOnGPU says).  Every SH option
                                 stays.  Draws restate SplatMaterial2D's vertex and fragment shaders (useRefImplementation =
                                 false): splat_scale, kernel2d, max_splat_px, GS_CAM_ANTIALIASED, GS_CAM_POINT_CLOUD and the
                                 per-scene opacity factor do not appear in that material and are ignored as it ignores them.
                                 Uploads, gs_mesh_project + a visibility-culled sort, gs_mesh_set_destination,
                                 gs_mesh_compute_distances, gs_mesh_bounds, trees, gs_mesh_remove / _reorder / _resize and the
                                 statistics work as for a 3D mesh.  GS_ERR_UNSUPPORTED, mesh unchanged: gs_mesh_set_draw_mode
                                 other than GS_DRAW_FP32, gs_mesh_debug_rop8, gs_mesh_surface, a camera with a tile-row strip,
                                 gs_group_render_gather.  gs_mesh_set_deep_pass is accepted and ignored (no deep pass) */

/* SplatMesh.build + setupDataTextures (SplatMesh.js:306-405, 637-898): device SoA planes instead of data
 * textures, so none of the 4096^2-texel limits apply. */
int gs_mesh_create(gs_context* ctx, uint32_t max_splat_count, uint32_t sh_degree, uint32_t flags,
                   gs_mesh** out);
void gs_mesh_destroy(gs_mesh* m);

/* Upload splats [from, from+count) in the formats fillSplatDataArrays emits (SplatMesh.js:1853-1902):
 *   centers float[3*count]
 *   cov     (m00,m01,m02,m11,m12,m22) per splat (SplatBuffer.js:440-486): cov_f32 float[6*count] for a
 *           full-precision mesh, cov_f16 uint16 (IEEE half bits)[6*count] for a GS_MESH_COV_HALF mesh -
 *           the caller narrows exactly as THREE.DataUtils.toHalfFloat does (SplatBuffer.js:469-474);
 *           exactly one of the two is non-NULL.  A GS_MESH_SURFEL mesh: cov_f32 carries (sx, sy, sz, qx, qy, qz) per splat, the
 *           tuple SplatMesh.updateScaleRotationsPaddedData stores (SplatMesh.js:1155-1170) - the scale (z already overridden to 1
 *           by the caller, as fillSplatDataArrays does in 2D mode, :1856-1863) and the x, y, z of the rotation normalised with
 *           w >= 0; the bound of what = 10 is then the largest squared scale, the spectral radius of the covariance the tuple
 *           stands for
 *   rgba    uint8[4*count]
 *   sh_f16  uint16 (IEEE half bits)[ncoef*count], coefficient-major RGB triples, ncoef = 0/9/24
 *           (SplatBuffer.js:680-728); NULL when the mesh has sh_degree 0. */
int gs_mesh_upload(gs_mesh* m, uint32_t from, uint32_t count, const float* centers, const float* cov_f32,
                   const uint16_t* cov_f16, const uint8_t* rgba, const uint16_t* sh_f16);

/* 8-bit SH of a GS_MESH_SH_U8 mesh: uint8[ncoef*count], same coefficient order as sh_f16 (pass sh_f16 = NULL to
 * gs_mesh_upload for such a mesh and call this for the same range). */
int gs_mesh_upload_sh_u8(gs_mesh* m, uint32_t from, uint32_t count, const uint8_t* sh_u8);

/* Decode splats [first, first+count) of an opened asset on the device and store them as splats
 * [from, from+count) of the mesh: the result is what gs_asset_fill(a, min_alpha, ...) followed by
 * gs_mesh_upload (+ gs_mesh_upload_sh_u8 for a level-2 file) of the same range leaves, plane for plane. Replaces
 * SplatBuffer.fillSplatCenterArray / fillSplatCovarianceArray / fillSplatColorArray / fillSphericalHarmonicsArray
 * (SplatBuffer.js:440-486, 517-734) + SplatMesh.updateDataTexturesFromBaseData (SplatMesh.js:900-1062) in one call:
 * the file's rows cross to the device, not the decoded arrays; a scene transform (gs_asset_set_transform) is applied
 * there too.  GS_ERR_INVALID, and nothing changes, when a range is
 * out of bounds, the mesh's SH degree differs from gs_asset_info.sh_degree, GS_MESH_SH_U8 disagrees with
 * sh_level == 2 for a degree > 0, or a GS_MESH_SURFEL mesh is handed an asset with a scene transform (as gs_asset_fill refuses
 * scales and rotations there).  Into a GS_MESH_SURFEL mesh the decode stores (sx, sy, 1, qx, qy, qz) per splat - bit for bit what
 * gs_asset_fill(..., scales, rotations), the scaleOverride.z = 1 of 2D mode and gs_mesh_upload leave.  GS_MESH_COV_HALF is the mesh's choice; the device narrows with
 * THREE.DataUtils.toHalfFloat's truncating rule (SplatBuffer.js:469-474). */
int gs_mesh_upload_asset(gs_mesh* m, uint32_t from, gs_asset* a, uint32_t first, uint32_t count, uint32_t min_alpha);

/* The `centers` message for the same range, derived on the device: int32 centres x1000 rounded as
 * SplatMesh.getIntegerCenters does (GS_SORT_INTEGER; SplatMesh.js:1912-1926), or the float centres
 * (getFloatCenters, :1935-1948), padFour.  scene_indexes as in gs_sorter_upload_centers.  Replaces
 * SplatBuffer.fillSplatCenterArray + getIntegerCenters / getFloatCenters + the worker's copy
 * (src/worker/SortWorker.js:84-98).  An asset with a scene transform gives the centres of the transformed fill.
 * GS_ERR_INVALID, and nothing changes, when a range is out of bounds or a GS_SORT_DYNAMIC sorter is handed an asset
 * with a transform (dynamic mode applies transforms per frame and never bakes them). */
int gs_sorter_upload_asset_centers(gs_sorter* s, uint32_t from, gs_asset* a, uint32_t first, uint32_t count,
                                   const uint32_t* scene_indexes);

/* Per-splat scene index (sceneIndexesTexture, SplatMesh.js:881-897): needed when more than one scene is loaded. */
int gs_mesh_upload_scene_indexes(gs_mesh* m, uint32_t from, uint32_t count, const uint32_t* scene_indexes);

/* Remove splats on the device (Viewer.removeSplatScenes without dispose + rebuild, src/Viewer.js:1326-1429).
 *   ranges       n_ranges pairs {from, count} in the caller's numbering: ascending, disjoint, non-empty, inside
 *                [0, max_splat_count], 1 <= n_ranges <= GS_MAX_SCENES.  Positions no upload has touched, or beyond the uploaded
 *                count, simply go away.  n_ranges == 0: GS_OK, nothing happens.
 *   scene_remap  NULL, or scene_remap_count <= GS_MAX_SCENES words (each < GS_MAX_SCENES): a surviving splat's scene index k
 *                becomes scene_remap[k] (k >= scene_remap_count: unchanged).  Send the surviving scenes' parameters again with
 *                gs_mesh_set_scenes.
 * Every surviving splat i becomes i - (removed positions below i); the uploaded count shrinks, the capacity and every allocation
 * stay.  No data crosses the bus: the storage spans of the survivors move down on the device.  A mesh in Morton storage order (no
 * GS_MESH_KEEP_ORDER) accepts a range only if neither of its borders falls inside a Morton run - the span of one fresh segment of
 * an upload (a first upload of [a, b) is one run); a GS_MESH_KEEP_ORDER mesh accepts any range.
 * Afterwards the mesh behaves, in every output, as a fresh mesh of the same capacity and flags that received the survivors by the
 * same uploads at their new positions.  The call waits for the mesh's work in flight and forgets what described the old numbering:
 * a pending gs_mesh_project, the last draw (gs_mesh_surface, gs_mesh_debug_rop8 and the draw's debug reads answer as before a
 * first draw), the statistics, and the resident result of every sorter bound to it.  Destination, draw mode and deep-pass switch
 * stay.  Trees are not edited: build a new one.  GS_ERR_INVALID, and nothing changes, on anything refused. */
int gs_mesh_remove(gs_mesh* m, const uint32_t* ranges, uint32_t n_ranges, const uint32_t* scene_remap, uint32_t scene_remap_count);

/* Fold the Morton runs that lie in [from, from + count) into ONE run, on the device: what a progressive load (one upload per
 * section, each a run of its own whose storage blocks span the scene) does at its final build.  Afterwards the mesh behaves, in
 * every output, as a fresh mesh of the same capacity and flags in which [from, from + count) arrived by one upload and every
 * other range by the uploads it did arrive by.  The caller's numbering does not change, no data crosses the bus, the capacity and
 * every allocation stay; splats outside the range keep their storage positions, the range keeps the storage slots
 * [from, from + count) and orders them as one upload would (bounds of its centres, 30-bit Morton codes, ties by index).
 * The call waits for the mesh's work in flight and forgets what described the old storage order: a pending gs_mesh_project, the
 * last draw (gs_mesh_surface, gs_mesh_debug_rop8 and the draw's debug reads answer as before a first draw), the statistics, and
 * the resident result of every sorter bound to it.  Destination, draw mode, deep-pass switch, scene parameters and trees stay
 * (they live in the caller's numbering).  The centre sums behind the motion heuristics stay as they are.
 * GS_OK and nothing happens - not even the last draw is forgotten - when count == 0, on a GS_MESH_KEEP_ORDER mesh, and when the
 * range holds at most one run.  GS_ERR_INVALID, and nothing changes, when from + count exceeds the uploaded count (on any mesh),
 * when a position of the range was never uploaded, or when a border of the range falls inside a Morton run (gs_mesh_remove's
 * rule). */
int gs_mesh_reorder(gs_mesh* m, uint32_t from, uint32_t count);

/* Change the capacity of a live mesh on the device: what adding a scene to a mesh that is already drawing needs
 * (Viewer.addSplatBuffersToMesh without dispose + rebuild, src/Viewer.js:1081-1141), and what gives memory back after a removal.
 *   max_splat_count  uploaded count <= max_splat_count <= 2^28 (gs_mesh_create's limit), larger or smaller than the current one.
 * Afterwards the mesh behaves, in every output, as a fresh mesh of the new capacity and the same flags that received the same
 * splats by the same uploads.  The caller's numbering, the uploaded count, the Morton runs, the storage positions, destination, draw
 * mode, deep-pass switch and scene parameters do not change; no splat data crosses the bus.  The first `uploaded` positions of every
 * resident plane are copied on the device, the positions behind them hold what gs_mesh_create leaves there (zero planes, the
 * identity permutation, boxes at the origin), and every buffer of the draw path that is sized by the capacity is allocated again
 * as gs_mesh_create (or its first user) allocates it.  The call waits for the mesh's work in flight and for the sorters bound to
 * it, and forgets what gs_mesh_remove forgets: a pending gs_mesh_project, the last draw, the statistics, and the resident result of
 * every sorter bound to it.  Trees are not edited.  Resize the sorter with gs_sorter_resize, in either order; between the two
 * calls a draw from a host list is safe.
 * GS_OK and nothing happens - not even the last draw is forgotten - when max_splat_count is the current capacity.
 * GS_ERR_INVALID, and nothing changes, for 0, a value above 2^28 or a value below the uploaded count (remove first).
 * GS_ERR_NOMEM when the new buffers cannot be allocated: everything the call allocated is released first, then the draw buffers
 * come back at the size they had - which needs no more memory than the mesh held before the call - and the mesh keeps its
 * capacity and its splats and stays usable (the last draw is forgotten).  Should even that fail, because another owner took the
 * memory meanwhile, the mesh keeps its splats but refuses draws, projections, uploads and gs_mesh_reorder (GS_ERR_INVALID) until
 * a gs_mesh_resize - to any accepted capacity, the present one included - succeeds. */
int gs_mesh_resize(gs_mesh* m, uint32_t max_splat_count);

/* Per-scene uniforms (SplatMesh.updateUniforms :1263-1276, setupDataTextures :868-878). */
typedef struct gs_scene_params {
    uint32_t scene_count;                       /* sceneCount                                                  */
    uint32_t pad;
    float transforms[GS_MAX_SCENES][16];        /* uniforms.transforms (GS_CAM_DYNAMIC)                        */
    float inv_cam_pos[GS_MAX_SCENES][4];        /* inverse(transform) * cameraPosition per scene; the shader
                                                   evaluates GLSL inverse() here (precision implementation-
                                                   defined), the caller passes the fp64 result               */
    float opacity[GS_MAX_SCENES];               /* sceneOpacity, clamped to [0,1]                              */
    uint32_t visible[GS_MAX_SCENES];            /* sceneVisibility                                             */
    float sh8_min[GS_MAX_SCENES];               /* sphericalHarmonics8BitCompressionRangeMin / Max             */
    float sh8_max[GS_MAX_SCENES];
} gs_scene_params;
int gs_mesh_set_scenes(gs_mesh* m, const gs_scene_params* params);

/* Uniforms of one draw: three's modelViewMatrix / projectionMatrix / cameraPosition plus
 * SplatMesh.updateUniforms (SplatMesh.js:1248-1280) as computed by Viewer.updateSplatMesh
 * (src/Viewer.js:651-677). */
typedef struct gs_camera {
    float view[16];          /* modelViewMatrix = viewMatrix * mesh.matrixWorld, column-major                */
    float proj[16];          /* projectionMatrix                                                            */
    float cam_pos[3];        /* cameraPosition                                                              */
    float focal[2];          /* focal.x/.y                                                                  */
    uint32_t width, height;  /* viewport in pixels (renderDimensions * devicePixelRatio)                    */
    float splat_scale;       /* setSplatScale, SplatMesh.js:1282                                            */
    float kernel2d;          /* kernel2DSize, default 0.3                                                   */
    float max_splat_px;      /* maxScreenSpaceSplatSize, default 1024 (src/Viewer.js:147)                   */
    float inv_focal_adj;     /* inverseFocalAdjustment                                                      */
    uint32_t sh_degree;      /* sphericalHarmonicsDegree uniform (<= mesh degree)                           */
    uint32_t flags;          /* GS_CAM_*                                                                    */
    uint32_t tile_row_begin; /* multi-GPU: this rank renders 16-px tile rows [begin,end); 0,0 = all rows    */
    uint32_t tile_row_end;
    /* shader permutations (all zero = static perspective scene) */
    float ortho_zoom;        /* orthoZoom (GS_CAM_ORTHOGRAPHIC)                                             */
    float scene_center[3];   /* sceneCenter (GS_CAM_FADE_IN)                                                */
    float fade_start_radius; /* visibleRegionFadeStartRadius (GS_CAM_FADE_IN)                               */
    float view_matrix[16];   /* viewMatrix (GS_CAM_DYNAMIC: modelView = viewMatrix * transforms[scene])     */
} gs_camera;
#define GS_CAM_ANTIALIASED 1u
#define GS_CAM_POINT_CLOUD 2u
#define GS_CAM_ORTHOGRAPHIC 4u   /* orthographicMode: J = diag(orthoZoom), SplatMaterial3D.js:112-117           */
#define GS_CAM_FADE_IN 8u        /* fadeInComplete == 0: distance fade-in, SplatMaterial.js:347-363             */
#define GS_CAM_SCENE_EFFECTS 16u /* enableOptionalEffects: per-scene opacity / visibility, SplatMaterial.js:129 */
#define GS_CAM_DYNAMIC 32u       /* dynamicMode: per-scene transforms, SplatMaterial.js:140-144,179-183         */
#define GS_TILE 16u
#define GS_DRAW_POOL_EXHAUSTED 1u   /* gs_render_stats.flags */

typedef struct gs_render_stats {
    float device_ms;          /* whole draw; the five times are 0 after a draw made without `stats` and
                                 without GS_CTX_STAGE_TIMING                                                 */
    float project_ms, bin_ms, tile_sort_ms, blend_ms;
    uint32_t visible_splats;  /* splats that survive the vertex-stage rejects                                */
    uint64_t tile_entries;    /* list entries = sum over splats of list bins (list_bin_px) touched           */
    uint32_t entry_capacity;
    uint32_t overflowed;      /* 1 = frame was re-run after growing the entry buffer                         */
    uint64_t tiles16;         /* D of SURVEY.md 8d = sum over splats of 16x16-px tiles touched               */
    uint32_t list_bin_px;     /* edge of a list bin of this draw (32, 128, 256 or 512): the unit of the entry lists and of
                                 gs_mesh_debug_read(what = 2); chosen per mesh from the previous measured draw    */
    uint32_t flags;           /* GS_DRAW_*: bit 0 = the per-bin blend ran out of chunk-partial slots (a list thousands of
                                 splats deep outside the deep pass): the affected quadrants were composited as one long chunk -
                                 still a valid front-to-back composite, but no longer bit-identical to what a strip of another
                                 cut or the deep pass would produce (was `pad`, always 0, before round 4)                    */
    uint64_t entries_scanned; /* list entries the blend read before its pixels saturated (<= tile_entries per 32-px
                                 bin of a list)                                                                  */
    uint64_t splats_walked;   /* (splat, 16x16-px tile) pairs the blend evaluated                                */
    uint64_t halves_evaluated; /* = 2 x splats_walked: both 16x8-px halves of a walked (splat, tile) pair are evaluated (the
                                 per-half skip of ABI 3's first draft was measured slower and removed; the field stays
                                 for layout compatibility)                                                         */
} gs_render_stats;

/* Entry-buffer overflow: a draw that returns statistics or pixels to the host checks and re-runs itself after growing the
 * buffers (gs_render_stats.overflowed).  A draw that returns nothing cannot; the following gs_mesh_render notices it without
 * synchronising, grows the buffers and returns GS_WARN_FRAME_TRUNCATED once.
 *
 * updateRenderIndexes(globalIndexes, renderSplatCount) + renderer.render(splatMesh, camera)
 * (SplatMesh.js:1228-1235, src/Viewer.js:1616).  Draw order = index order = back-to-front.
 *   sorted_host   uint32[render_count] host, or NULL
 *   sorter        take the device-resident result of the last gs_sorter_sort (when sorted_host == NULL)
 *   rgba_out_host uint8[4*W*rows*16...] RGBA8, row 0 = bottom (GL), covering tile rows [begin,end) clipped
 *                 to the viewport; or NULL
 *   rgba_out_dev  same, device pointer (e.g. a torch uint8 tensor); or NULL to use an internal buffer */
int gs_mesh_render(gs_mesh* m, const gs_camera* cam, const uint32_t* sorted_host, gs_sorter* sorter,
                   uint32_t render_count, uint8_t* rgba_out_host, void* rgba_out_dev, gs_render_stats* stats);

/* The DESTINATION the splats are blended into.  The reference draws the other scene geometry first and then the splats with
 * `depthTest: true, depthWrite: false` and NormalBlending (src/splatmesh/SplatMaterial3D.js:72-73; draw order
 * src/Viewer.js:1610-1616; drop-in mode, where the splat mesh is one object of the host's own scene:
 * src/DropInViewer.js:34-42): a splat fragment is kept where its depth passes three's default depthFunc (LessEqualDepth)
 * against the depth the opaque geometry left, and what is kept is blended OVER the colour that geometry left.  The quad of a
 * splat sits at its centre's depth (gl_Position.z = ndcCenter.z, SplatMaterial3D.js:206-210), so the test is per (splat,
 * pixel): window depth of the splat's CENTRE, 0.5 * ndc.z + 0.5 (glDepthRange 0..1), <= depth[pixel].
 *
 *   depth_host / depth_dev   float[height * width], window-space depth in [0, 1] as glReadPixels(DEPTH_COMPONENT, FLOAT) or
 *                            a THREE.DepthTexture(FloatType) holds it, row 0 = bottom; at most one of the two; both NULL = no
 *                            depth test (every fragment passes)
 *   rgba_host / rgba_dev     uint8[4 * height * width] RGBA8, row 0 = bottom: the colour the splats are blended over
 *                            (rgb = C + T * dst.rgb, alpha = 1 - T * (1 - dst.a): what NormalBlending, back to front, leaves);
 *                            both NULL = the reference Viewer's clear colour (0, 0, 0, 0)
 *   width, height            must equal the camera's viewport at every draw while the destination is set
 *   GS_DEST_DEPTH_UNORM24    compare as a 24-bit fixed-point depth buffer does: both sides round(z * (2^24 - 1)) first
 *
 * Host buffers are copied to the device by this call (it returns when they are reusable); device buffers are READ BY EVERY
 * FOLLOWING DRAW until the destination is replaced or cleared (dest == NULL) - the caller keeps them alive and orders its
 * writes to them before the draws (same stream or an event).  A multi-GPU strip reads its own rows of the full-size buffers.
 * Draw modes and outputs are unchanged; frames stay bit-identical across strips and across the deep pass.
 * The call waits for the mesh's draws in flight (they read the previous destination).  A descriptor that is refused (both a host
 * and a device pointer for one plane, unknown flags, a size of 0 or beyond 65536 px) leaves the mesh WITHOUT a destination. */
#define GS_DEST_DEPTH_UNORM24 1u
typedef struct gs_destination {
    const float* depth_host;
    const void* depth_dev;
    const uint8_t* rgba_host;
    const void* rgba_dev;
    uint32_t width, height;
    uint32_t flags;
    uint32_t pad;
} gs_destination;
int gs_mesh_set_destination(gs_mesh* m, const gs_destination* dest);

/* The vertex stage of a draw on its own (the GLSL vertex shader, SplatMaterial.js:112-341 + SplatMaterial3D.js:81-217):
 * projects every uploaded splat for `cam` and leaves records, tile rects and the visibility mask on the device.  The next
 * gs_mesh_render with an identical gs_camera consumes them instead of projecting again (once: the vertex stage runs exactly
 * one time per frame either way); any other camera simply projects afresh.  Needed before a visibility-culled sort. */
int gs_mesh_project(gs_mesh* m, const gs_camera* cam);

/* The distance pass of gpuAcceleratedSort: SplatMesh.computeDistancesOnGPU (SplatMesh.js:1701-1814) with the transform-feedback
 * vertex shader of :1449-1490, over every uploaded splat, one value per ORIGINAL splat index.
 *   flags     GS_SORT_INTEGER (integerBasedDistancesComputation) | GS_SORT_DYNAMIC (dynamicMode)
 *   uniforms  exactly what the reference uploads:
 *               static integer   int32[3]               getIntegerMatrixArray(mvp)[2, 6, 10]
 *               static float     float[3]               mvp.elements[2, 6, 10]
 *               dynamic integer  int32[4 * scene_count] getIntegerMatrixArray(mvp * scene.transform)[2, 6, 10, 14] per scene
 *               dynamic float    float[16 * scene_count] (mvp * scene.transform).elements per scene, column-major
 *             (getIntegerMatrixArray = Math.round(m * 1000) per element, SplatMesh.js:2057-2064, then WebGL's int32 conversion)
 *   scene_count  1..GS_MAX_SCENES (static: 1); scenes beyond it read zero rows, like unset GL uniforms
 *   out_host  int32 / float[uploaded splats] by original index (waits for it), or NULL
 *   dst       a sorter of the same context whose device-side precomputed-distance buffer receives the result (no PCIe; the
 *             next gs_sorter_sort / _gathered with precomputed = GS_PRECOMPUTED_DEVICE sorts it), or NULL.  Its max_splat_count
 *             must cover the mesh's uploaded splats.  The hand-over is ordered with an event on a multi-stream context.
 * Arithmetic per splat at storage position p (centres as gs_mesh_upload received them, in fp32):
 *   integer   x, y, z = ToInt32(Math.round((double)c * 1000)) (getIntegerCenters(padFour), SplatMesh.js:1912-1926: NaN and
 *             infinities -> 0, everything else wraps modulo 2^32), w = 1000; products and sums wrap modulo 2^32 (GLSL ES 3.00)
 *               static   x*u.x + y*u.y + z*u.z                      dynamic  x*t.x + y*t.y + z*t.z + t.w*1000
 *   float     fp32, every product and sum rounded on its own (no fused multiply-add), left to right
 *               static   ((x*u.x + y*u.y) + z*u.z)                  dynamic  (((T[2]*x + T[6]*y) + T[10]*z) + T[14])
 *             (a GL driver may contract these, so the reference itself is defined to within an ulp here)
 * GS_ERR_INVALID for unknown flags, scene_count 0 or > GS_MAX_SCENES, a dynamic pass over several scenes on a mesh without scene
 * indexes, or a dst smaller than the mesh's uploaded splat count. */
int gs_mesh_compute_distances(gs_mesh* m, uint32_t flags, const void* uniforms, uint32_t scene_count, void* out_host,
                              gs_sorter* dst);
/* `precomputed` argument of gs_sorter_sort / gs_sorter_sort_gathered: sort the distances the last gs_mesh_compute_distances(...,
 * dst = this sorter) left on the device (nothing crosses PCIe).  GS_ERR_INVALID when the sorter never received any, received fewer
 * than its uploaded splat count, or received them for the other GS_SORT_INTEGER setting.  A sort with host distances overwrites
 * them. */
#define GS_PRECOMPUTED_DEVICE ((const void*)(uintptr_t)1)

/* Intermediates of the last draw (tests, strip load-balancing).  what: 0 = per splat (storage order) the
 * 32-byte vertex-stage record {cx, cy, ax, ay, bx, by, r|g<<16, b|a<<16 (unorm16)}; 1 = per splat the tile
 * rect {x0|y0<<16, x1|y1<<16} (0 and 1 are defined only for splats whose mask bit is set); 2 = per list bin (gs_render_stats.list_bin_px) of the
 * drawn strip the [begin,end) range of its entry list ((~0,0) = untouched); 3 = the visibility mask, 1 bit per
 * splat packed in uint64 words (count = number of words); 4 = per 32x32-px blend bin of the drawn strip (row-major,
 * bins_x = ceil(width / 32)) the pair {list entries scanned, 2 x (splat, 16x16-px quadrant) pairs composited}: the blend's
 * real cost, used to balance multi-GPU strips; 5 = the deep pass of the last draw: {bins it composited, bins over its threshold,
 * chunk partials the per-bin kernel closed itself, 1 if that pool ran out}, then the bin numbers (count = 4 .. 4 + 512 words);
 * 6 = host state (count = 3 or 4 words): {visible splats, splats projected} of the last full-frame draw whose verdict has reached the
 * host, where the last vertex stage ran its block test (1 = a kernel of its own, 0 = in every workgroup, 2 = not at all), and - with
 * count = 4 - which k_project instance that stage launched: bit 0 = the shader-permutation kernel (orthographic, fade-in, scene
 * effects, per-scene transforms, 8-bit SH, several scenes), bit 1 = it wrote window depths (a destination depth), bit 2 = the 4-byte
 * look-up word, bit 3 = the surfel kernel of a GS_MESH_SURFEL mesh (k_project_2d) instead of k_project;
 * 7 = the blend schedule of the last draw (the one workgroup that orders the blend's bins by the previous draw's per-bin statistics,
 * what = 4, and names the deep pass's members), GS_SCHEDULE_WORDS words: {1 if it ran, blend bins, shift x, shift y (int32: this
 * draw's bin (x, y) reads the statistics of bin (x - sx, y - sy)), 1 if this draw ran the deep pass, deep_min, deep_factor, bit 0:
 * the blend visited its bins in that order (other bits reserved, 0), the bins it put over the deep pass's trigger (0 when none reached it), the members' share of the walk in
 * 1/1024}, then the bin order itself (count = GS_SCHEDULE_WORDS .. + blend bins; the order only after a draw that ran it);
 * 8 = the entry values of the last draw in list order: `count` uint32 record slots (count <= min(tile_entries, entry_capacity) of
 * that draw), the array the [begin,end) ranges of what = 2 index, each list near -> far; refused while a gs_mesh_project is pending
 * (the slots then refer to the other record set, as for gs_mesh_debug_rop8);
 * 9 = per splat, in the caller's numbering, the record slot the last vertex stage gave it (uint32, 0xFFFFFFFF = not visible): what
 * the entries of what = 8 name a splat by;
 * 10 = per splat, in the caller's numbering, the bound of its covariance's spectral radius that the strip pre-tests read (float;
 * count <= the uploaded splats); 11 = the boxes of the 256-splat storage blocks, 8 floats per block: {min xyz, max xyz of the
 * members' centres (NaN left out), the largest member bound of what = 10 (NaN if any member's is), unused} (count = blocks <=
 * ceil(max_splat_count / 256)); 12 = per splat, in the caller's numbering, its storage position (uint32; block = position / 256).
 * 13 = the window depths the last draw's destination depth test compared, float per RECORD SLOT (what = 9 gives a splat's slot; only
 * the slots of visible splats are defined; count <= max_splat_count): 0.5 * ndc.z + 0.5 as the vertex stage formed it, or that value as
 * a 24-bit integer under GS_DEST_DEPTH_UNORM24; refused when the last draw had no destination depth.
 * 15 = (GS_MESH_SURFEL meshes only, which in turn refuse what = 0) per splat, in the caller's numbering, the 80-byte vertex-stage
 * record of a surfel, 20 words: vT as Tu xyz, Tv xyz, Tw xyz (SplatMaterial2D.js:125); vQuadCenter xy; the quad's centre in pixels;
 * the inverse i00, i01, i10, i11 of the quad's 2x2 basis in pixels (pixel centre f is inside iff |i00 dx + i01 dy| <= 1 and
 * |i10 dx + i11 dy| <= 1, d = f - centre); r|g<<16, b|a<<16 (unorm16); one unused word.  Zeros where the mask bit is clear.
 * 10 .. 12 read what the uploads left and need no draw.  Like the reads above, 10 and 12 go through the mesh's upload staging
 * buffer: no debug read may run while another thread uploads to the same mesh.
 *
 * The composite (csrc/tile_blend.hip).  Per 16x16-px quadrant, the ordered list entries whose ellipse reaches the quadrant are
 * cut into chunks of 1024; a chunk is the plain front-to-back composite from T = 1, and the chunks are merged near -> far
 * (C = fma(T, C_c, C); T = T * T_c).  Up to 1024 contributing splats per quadrant - every quadrant of the BASELINE
 * configurations - that is exactly the single front-to-back composite; beyond, it differs from it by fp32 rounding, and it lets
 * many waves composite one very deep quadrant at once (the "deep pass", chosen per bin from the previous draw's statistics).
 * The frame does not depend on that choice, on list batching or on how a multi-GPU draw cuts its strips. */
#define GS_SCHEDULE_WORDS 10
int gs_mesh_debug_read(gs_mesh* m, int what, void* dst, uint32_t count);

/* VERIFICATION of the blend state (SplatMaterial3D.js:65-75): the reference composites back to front into an RGBA8 target,
 * rounding every channel to 8 bits after EVERY splat; gs_mesh_render composites front to back in fp32 and rounds once.  This
 * entry point reproduces the reference's own semantics for a window of <= 65536 pixels of the LAST draw (its lists, records
 * and camera): rgb = a*src + (1-a)*rgb, alpha = a + (1-a)*alpha, then floor(clamp01(v)*255 + 0.5) per channel, splat by
 * splat, farthest first.  (x0, y0) in GL window coordinates (row 0 = bottom), inside the rows the last draw covered;
 * rgba_out_host: uint8[4*width*height], row-major from y0 upwards.  A thread per pixel walks its whole list: not a draw mode. */
int gs_mesh_debug_rop8(gs_mesh* m, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint8_t* rgba_out_host);

/* THE SURFACE PASS: where the splat surface of the LAST draw is, per pixel of a window - what a host scene that draws AFTER the
 * splats needs (transparent objects, a cursor, depth of field, collision, click-to-focus).  For the pixel centred at
 * (px + 0.5, py + 0.5) the entry list of its list bin is walked near -> far; an entry is KEPT when its 16-px tile rect covers the
 * pixel's tile, the fragment rule keeps it (power < 4 log2(e), i.e. A <= 8, as in the blend) and - when the last draw had a
 * destination depth - its window depth passes the blend's test against the stored depth (GS_DEST_DEPTH_UNORM24 included: splats
 * hidden by opaque geometry are not surface).  Each kept entry contributes a = exp2(-power) * alpha in the blend's own fp32
 * arithmetic; from T = 1, T <- T (1 - a).  The answer is the FIRST kept entry after which T <= threshold - the "median depth" of
 * the 3DGS literature at threshold 0.5:
 *   ids    that splat's index in the caller's numbering, 0xFFFFFFFF when the list ends first;
 *   depth  the window depth of that splat's centre, 0.5 * ndc.z + 0.5 as an unquantised float (the vertex stage's expression
 *          order, per-scene transforms of GS_CAM_DYNAMIC included, read as they are set NOW), 1.0f when there is none.
 * (x0, y0) in GL window coordinates (row 0 = bottom); the window is 1x1 .. the whole frame and lies inside the rows the last
 * draw covered (a strip draw covers only its own rows).  Outputs: row-major from y0 upwards, `width` per row; any subset of the
 * four pointers, at least one, and not a host and a device pointer for the same plane.  Host outputs wait for the result; device
 * outputs only enqueue on the context's stream.  The answer does not depend on the window, on list batching, on the list-bin size,
 * on the storage order or on how strips cut the frame.  The mesh must still hold the splats that draw saw: an upload or new scene
 * parameters between the draw and this call are not detected, and the ids and depths then describe the new contents.
 * GS_ERR_INVALID, nothing written: no draw yet; a gs_mesh_project is pending; the destination changed since the last draw; a
 * threshold outside (0, 1) or NaN; an empty window or one that leaves the drawn rows; no output; both pointers of a plane.
 * Cost (csrc/tile_blend.hip, k_surface): a workgroup per 32-px bin of the window, a wave per 16x16 quadrant, lists scanned in
 * batches of 256 until every pixel of the bin has its answer - a few splats deep where the frame is opaque.  Translucent content
 * that never reaches the threshold is walked to the end of its list by ONE wave per quadrant: there is no chunked or deep path
 * here.  No existing kernel takes part: frames are unchanged. */
int gs_mesh_surface(gs_mesh* m, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, float threshold,
                    uint32_t* ids_out_host, float* depth_out_host, void* ids_out_dev, void* depth_out_dev);

/* SCENE BOUNDS: where the splats [from, from + count) of the caller's numbering are - the reference's two host loops over every
 * centre, as one read-only device pass over the planes the mesh keeps (csrc/bounds.hip):
 *   SplatMesh.updateVisibleRegion  (src/splatmesh/SplatMesh.js:1172-1199)  max over the range of |c - center|, which drives the
 *                                  scene fade-in (GS_CAM_FADE_IN: gs_camera::scene_center / fade_start_radius);
 *   SplatMesh.computeBoundingBox   (:2066-2095)                            min / max of the centres as a Float32Array holds them.
 * c is the stored fp32 centre widened to double, or - GS_BOUNDS_TRANSFORM - transforms[scene of the splat] applied to it first
 * exactly as THREE.Vector3.applyMatrix4 writes it: w = 1 / (e3 x + e7 y + e11 z + e15), x' = (e0 x + e4 y + e8 z + e12) w, ...;
 * the scene comes from the plane gs_mesh_upload_scene_indexes filled (none: every splat is scene 0; an index >= scene_count: 0).
 * Every product, sum and the division is one fp64 operation in the reference's order, d = c - center per component, then
 * (dx dx + dy dy) + dz dz: Vector3.sub(...).length() without the root.  The caller takes the root: sqrt is monotone and correctly
 * rounded, so sqrt(max s) == max sqrt(s) bit for bit.  The box takes (float)x' - the Float32Array store - the distance the
 * unrounded double.  The maximum uses `d > m` from 0, the box `<` and `>`; a splat with a NaN component (after the transform)
 * takes part in neither and is not counted - the reference differs only when splat 0 is NaN (its box starts from splat 0
 * unconditionally); +-Inf propagates.  Minimum and maximum are exact, so the result does not depend on the launch geometry or on
 * the storage order (GS_MESH_KEEP_ORDER).
 * Bit-equal to the reference's running maximum wherever the mesh's stored centres are the floats the reference reads (a level-0
 * buffer with no or an identity baked transform; dynamic mode with GS_BOUNDS_TRANSFORM).  Where the reference keeps an unrounded
 * double and the mesh its Float32Array rounding (a baked non-identity static transform, .ksplat level 1 / 2 bucket decoding,
 * SplatBuffer.js:232-246) the radius differs by at most 2^-24 (R + |center|): half an ulp per component is |e| <= 2^-24 |c|, and
 * | |a + e| - |a| | <= |e|.
 * count == 0: GS_OK, every field 0.  A range that is not wholly uploaded: GS_ERR_INVALID, *out untouched.  The call enqueues
 * behind the mesh's uploads on the context's stream, waits and returns; it writes none of the mesh's planes, so draws in flight
 * are not disturbed.  No existing kernel takes part: frames are unchanged. */
#define GS_BOUNDS_TRANSFORM 1u
typedef struct gs_bounds {
    uint64_t count;                /* splats of the range that took part                                            */
    float box_min[3], box_max[3];  /* 0 when count == 0                                                             */
    double max_dist_sq;            /* max |c - center|^2 over them; 0 for none                                      */
} gs_bounds;
int gs_mesh_bounds(gs_mesh* m, uint32_t from, uint32_t count, const double* center, const double* transforms,
                   uint32_t scene_count, uint32_t flags, gs_bounds* out);

/* DRAW MODE of the draws that follow.
 *   GS_DRAW_FP32 (default)  the front-to-back fp32 composite, rounded to RGBA8 once (early termination, chunks, the deep pass):
 *                           <= 0.52 / 255 from the exact composite, 3-4 / 255 from what a browser's RGBA8 target shows on
 *                           translucent content (tests/test_gpu_crops.py gates both).
 *   GS_DRAW_ROP8_FULL       the reference's own blend state as it executes on a GPU (SplatMaterial3D.js:65-75: NormalBlending into
 *                           an RGBA8 target; src/Viewer.js:358-359: cleared to (0,0,0,0), or the destination's colour): back to
 *                           front, rgb = a*src + (1-a)*rgb, alpha = a + (1-a)*alpha, every channel rounded to 8 bits after EVERY
 *                           splat - gs_mesh_debug_rop8's semantics for the whole frame: >= 99.85 % of the channel values equal to
 *                           the ROP-emulating oracle, never more than 1 apart.  Every list is walked whole (no early termination
 *                           is possible back to front): the blend of a 1080p garden frame takes 4.0 ms instead of 0.06.
 *   GS_DRAW_ROP8            the same composite over the splats IN FRONT OF each 16x16 quadrant's saturation depth only: a first
 *                           pass walks the list front to back until every pixel of the quadrant has let <= 1e-6 through (counting
 *                           fragments of alpha >= 1/64: fainter ones hide nothing from an 8-bit target), a second pass blends
 *                           exactly those splats back to front with the per-splat rounding.  Colour: the full walk's gate
 *                           (>= 99.5 % of the r, g, b values equal to the ROP-emulating oracle, never more than 1 apart; on the
 *                           C3T crops colour is identical to the full walk).  Alpha: exact wherever it reaches 255; where it
 *                           stalls below 255 - alpha = q8(a + (1-a) alpha) stops moving once a (255 - alpha) < 0.5 - the value
 *                           it stalls at depends on the whole list and may differ by <= 2 steps.  Garden stand-in at 1080p:
 *                           blend 0.32 ms, i.e. a 0.50 ms frame = 11.6 Gsplats/s with the browser's colours; translucent content
 *                           (nothing saturates) costs what the full walk costs.
 * Strips, destinations (depth test and colour) and device-resident outputs work as in the fp32 mode; the statistics count the pairs
 * the mode walked, and they never schedule a later fp32 draw. */
#define GS_DRAW_FP32 0u
#define GS_DRAW_ROP8 1u
#define GS_DRAW_ROP8_FULL 2u
int gs_mesh_set_draw_mode(gs_mesh* m, uint32_t mode);

/* Scheduling switch, 1 by default (0 also via $GSPLAT_NO_DEEP at gs_mesh_create): whether the draws that follow may composite
 * very deep bins through the deep pass.  The frame is the same either way (see the composite above). */
int gs_mesh_set_deep_pass(gs_mesh* m, int enabled);

/* Measurement hook: summed device duration (HIP events on the stream the kernel is launched on) and number of
 * launches since the last reset.  which: 0 = k_project alone (the sampled untimed draws), 1 = the whole vertex stage (block
 * test + mask reset + k_project) of the timed draws - two clocks, kept apart.  Synchronises the streams.
 * On a single-stream context without GS_CTX_STAGE_TIMING every 8th launch is measured ($GSPLAT_KERNEL_SAMPLE; the two event
 * records cost 1.5 % of a frame): `launches` counts the measured ones. */
int gs_mesh_kernel_time(gs_mesh* m, int which, int reset, double* sum_ms, uint32_t* launches);

/* ------------------------------------------------------------------------------------------------ *
 * MULTI-GPU: tile-row strips, one rank per GPU, strips gathered over RCCL (no counterpart in the reference)
 * ------------------------------------------------------------------------------------------------ */
typedef struct gs_group gs_group;
#define GS_GROUP_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank and hand the 128 bytes to every rank (any side channel: MPI, a file, a pipe). */
int gs_group_unique_id(uint8_t* id_out);
/* ncclCommInitRank on the context's device.  Collective: every rank of the group calls it with the same id.
 * world_size 1 needs no id and never loads RCCL. */
int gs_group_create(gs_context* ctx, const uint8_t* id, uint32_t world_size, uint32_t rank, gs_group** out);
void gs_group_destroy(gs_group* g);
/* Gatherv of framebuffer strips, enqueued on the context's stream (returns without waiting).  Rank r owns pixel rows
 * [row_begin[r], row_end[r]) of a `width`-pixel RGBA8 frame (GL row order, as gs_mesh_render writes a strip: its first row
 * is row_begin[r]); strip_dev = this rank's rows, full_dev = the whole frame on `root` (ignored elsewhere).  Collective. */
int gs_group_gather_strips(gs_group* g, const void* strip_dev, void* full_dev, uint32_t width, const uint32_t* row_begin,
                           const uint32_t* row_end, uint32_t root);
/* Overlapped gathers (off by default).  The strips of an 8K frame are 133 MB: the root receives 16.6 MB from each of 7 peers
 * (~0.25 ms over one xGMI link each; with 2 ranks 66 MB over ONE link, ~0.9 ms) - as long as a rank's whole frame.  With
 * overlap on, gs_group_gather_strips / gs_group_render_gather enqueue the transfer on a stream of the group: it starts when
 * everything enqueued on the context's stream so far (the draw of this frame) has finished, and runs while the context's
 * stream goes on with the next frame.  Contract: the caller ALTERNATES between two strip buffers and two full-frame buffers
 * (gs_group_render_gather does that itself; its root's frame alternates between two internal buffers too); call k makes the
 * context's stream wait for the transfer of call k-1, so the draw that follows may overwrite the buffers of call k-1's
 * predecessor.  gs_group_wait blocks the host until every transfer issued so far has completed (the root's consumer calls it -
 * or synchronises the device - before it reads a gathered frame).  Every rank of the group must use the same setting. */
int gs_group_set_overlap(gs_group* g, int enabled);
int gs_group_wait(gs_group* g);

/* One rank's whole share of a multi-GPU draw: gs_mesh_render (same sorted_host | sorter choice) of its strip (pixel rows [row_begin[rank], row_end[rank]),
 * whole 16-px tile rows; `cam` describes the full viewport) into the mesh's own device framebuffer, then the gather above.
 * On `root`, rgba_out_host (nullable) receives the full W*H*4 frame (this waits for it); the other ranks only enqueue.
 * With gs_sorter_set_visibility_cull call gs_mesh_project with the same strip in the camera first.  Collective. */
int gs_group_render_gather(gs_group* g, gs_mesh* m, const gs_camera* cam, const uint32_t* sorted_host, gs_sorter* sorter, uint32_t render_count,
                           const uint32_t* row_begin, const uint32_t* row_end, uint32_t root, uint8_t* rgba_out_host);

/* Statistics of the last draw (synchronises the stream). */
int gs_mesh_last_stats(gs_mesh* m, gs_render_stats* stats);
/* Test hook: shrink (or grow) the entry buffers so a small scene can exercise the overflow -> regrow path. */
int gs_mesh_debug_set_entry_capacity(gs_mesh* m, uint32_t capacity);
int gs_sorter_last_stats(gs_sorter* s, gs_sort_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_HIP_H */
