// mesh_edit.hip — removing splats from a live mesh on the device (gs_mesh_remove), and the plane compaction the sorter's half
// (sorter.hip, gs_sorter_remove) shares.  Replaces the dispose + rebuild of Viewer.removeSplatScenes
// (the reference's src/Viewer.js:1326-1429) for the device objects: the survivors' storage spans move down, nothing crosses the bus.
// Which spans move where, and which calls are refused, is upload_plan.hpp's (plan_remove); DESIGN.md 8.13.
// Second half of the file: gs_mesh_reorder, which folds the Morton runs of a range - one per fresh upload, as a progressive load leaves
// them - into the one run a single upload would have been (plan_reorder).
// Between the two: gs_mesh_resize and the move both resize calls share (gs_capacity_move).
#include <algorithm>

#include "gs_internal.hpp"

static_assert(REMOVE_MAX_RANGES == GS_MAX_SCENES, "one removed range per scene");

// ---------------------------------------------------------------------------------------------------
// The move.  Source and destination of a span overlap whenever it is longer than its shift, so a plane is never moved in place:
// one launch gathers every position from `base` to the new end into a scratch buffer (16 bytes per position at most: the
// staging buffer), one copy between the two distinct buffers puts them back.  No workgroup waits for another, no copy overlaps
// itself, and the launches are per plane, not per range: the <= 32 cuts travel as kernel arguments (scalar registers).
// ---------------------------------------------------------------------------------------------------
RemoveMap gs_remove_map(const RemovePlan& p, const uint32_t* scene_remap, uint32_t scene_remap_count) {
    RemoveMap r = {};
    r.n = (uint32_t)p.cuts.size();
    uint32_t cum = 0;
    for (uint32_t k = 0; k < r.n; k++) {
        r.old_begin[k] = p.cuts[k].begin;
        r.new_begin[k] = p.cuts[k].begin - cum;
        cum += p.cuts[k].end - p.cuts[k].begin;
        r.cum[k] = cum;
    }
    for (uint32_t k = 0; k < GS_MAX_SCENES; k++) r.scene[k] = (scene_remap && k < scene_remap_count) ? scene_remap[k] : k;
    return r;
}

// removed positions below the survivor that lands on NEW position j (the cuts are uniform: scalar loads and compares)
__device__ __forceinline__ uint32_t removed_below_new(const RemoveMap& r, uint32_t j) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < r.n; k++) s = j >= r.new_begin[k] ? r.cum[k] : s;
    return s;
}
// ... below the survivor at OLD position v
__device__ __forceinline__ uint32_t removed_below_old(const RemoveMap& r, uint32_t v) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < r.n; k++) s = v >= r.old_begin[k] ? r.cum[k] : s;
    return s;
}

// scratch[g] = the 16 bytes of new positions base + g * V .. + V of a plane of T (V = 16 / sizeof(T); zeros beyond n_out).
// MODE: GS_REMOVE_PLAIN the elements as they are | GS_REMOVE_POSITIONS they are positions (perm, inv_perm): index space and
// storage space share one shift function under the run rule | GS_REMOVE_SCENES they are scene indexes: through the table
template <class T, int MODE>
__global__ __launch_bounds__(256) void k_remove_gather(const T* __restrict__ plane, uint32_t base, uint32_t n_out, RemoveMap r,
                                                       uint4* __restrict__ scratch) {
    constexpr uint32_t V = 16u / sizeof(T), W = sizeof(T) / 4u;      // elements per 16 bytes, words per element
    static_assert(MODE == GS_REMOVE_PLAIN || W == 1u, "positions and scene indexes are words");
    const uint32_t groups = (n_out + V - 1u) / V;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t t = 0; t < V; t++) {
            const uint32_t o = g * V + t;
            if (o >= n_out) continue;
            const uint32_t j = base + o;
            __builtin_memcpy(&w[t * W], &plane[j + removed_below_new(r, j)], sizeof(T));   // (one load of the element's size)
            if constexpr (MODE == GS_REMOVE_POSITIONS) w[t] -= removed_below_old(r, w[t]);
            if constexpr (MODE == GS_REMOVE_SCENES) w[t] = w[t] < GS_MAX_SCENES ? r.scene[w[t]] : w[t];
        }
        scratch[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ __launch_bounds__(256) void k_remove_iota(uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint32_t from, uint32_t end) {
    for (uint32_t i = from + blockIdx.x * blockDim.x + threadIdx.x; i < end; i += gridDim.x * blockDim.x) a[i] = b[i] = i;
}

static inline uint32_t edit_grid(uint32_t n) {
    const uint32_t g = (n + 255u) / 256u;
    return g < 1u ? 1u : (g > 4096u ? 4096u : g);
}

// One plane: positions [base, new_end) gathered and put back, [new_end, old_end) zeroed (what a fresh object holds there).
// scratch holds >= 16 * (new_end - base) + 16 bytes.  Enqueued on st; the caller checks hipGetLastError.
int gs_remove_compact(hipStream_t st, const RemoveMap& map, void* plane, uint32_t elem_bytes, int mode, uint32_t base, uint32_t new_end,
                      uint32_t old_end, void* scratch) {
    if (!plane) return GS_OK;
    const uint32_t n_out = new_end - base;
    if (n_out) {
        const dim3 g(edit_grid((uint32_t)(((size_t)n_out * elem_bytes + 15u) / 16u))), b(256);
        uint4* sc = static_cast<uint4*>(scratch);
        if (elem_bytes == 16) hipLaunchKernelGGL((k_remove_gather<uint4, GS_REMOVE_PLAIN>), g, b, 0, st, (const uint4*)plane, base, n_out, map, sc);
        else if (elem_bytes == 8) hipLaunchKernelGGL((k_remove_gather<uint2, GS_REMOVE_PLAIN>), g, b, 0, st, (const uint2*)plane, base, n_out, map, sc);
        else if (mode == GS_REMOVE_POSITIONS)
            hipLaunchKernelGGL((k_remove_gather<uint32_t, GS_REMOVE_POSITIONS>), g, b, 0, st, (const uint32_t*)plane, base, n_out, map, sc);
        else if (mode == GS_REMOVE_SCENES)
            hipLaunchKernelGGL((k_remove_gather<uint32_t, GS_REMOVE_SCENES>), g, b, 0, st, (const uint32_t*)plane, base, n_out, map, sc);
        else hipLaunchKernelGGL((k_remove_gather<uint32_t, GS_REMOVE_PLAIN>), g, b, 0, st, (const uint32_t*)plane, base, n_out, map, sc);
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpyAsync(static_cast<char*>(plane) + (size_t)base * elem_bytes, scratch, (size_t)n_out * elem_bytes, hipMemcpyDeviceToDevice, st));
    }
    if (old_end > new_end)
        GS_HIP(hipMemsetAsync(static_cast<char*>(plane) + (size_t)new_end * elem_bytes, 0, (size_t)(old_end - new_end) * elem_bytes, st));
    return GS_OK;
}

// The centre sums of positions [0, n) (gs_mesh::centre_sum / centre_sq / centre_n: a heuristic's inputs, not pinned): per
// workgroup {x, y, z, x*x + y*y + z*z, count} in fp64.  Never-uploaded positions inside [0, n) count as the zero centres they hold.
constexpr uint32_t CENTRE_SUM_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_remove_centre_sums(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                            uint32_t n, double* __restrict__ out) {
    __shared__ double s_part[4][5];
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float x = px[i], y = py[i], z = pz[i];
        const float r2 = x * x + y * y + z * z;
        if (!(r2 < 1e30f)) continue;                          // NaN / infinite centres draw nothing
        s[0] += x; s[1] += y; s[2] += z; s[3] += r2; s[4] += 1.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 5; k++) s[k] += __shfl_xor(s[k], o, 64);
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 5; k++) s_part[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x < 5u) out[5u * blockIdx.x + threadIdx.x] = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

static int mesh_recount_centres(gs_mesh* m) {
    m->centre_sum[0] = m->centre_sum[1] = m->centre_sum[2] = m->centre_sq = 0.0;
    m->centre_n = 0;
    if (m->uploaded == 0) return GS_OK;
    hipStream_t st = m->ctx->stream;
    double part[CENTRE_SUM_BLOCKS * 5];
    const uint32_t blocks = std::min((m->uploaded + 255u) / 256u, CENTRE_SUM_BLOCKS);
    GS_TRY(m->staging.ensure(sizeof(part)));
    hipLaunchKernelGGL(k_remove_centre_sums, dim3(blocks), dim3(256), 0, st, m->px.as<float>(), m->py.as<float>(), m->pz.as<float>(), m->uploaded,
                       m->staging.as<double>());
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(part, m->staging.p, sizeof(double) * 5 * blocks, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    for (uint32_t b = 0; b < blocks; b++) {
        for (int k = 0; k < 3; k++) m->centre_sum[k] += part[5 * b + k];
        m->centre_sq += part[5 * b + 3];
        m->centre_n += (uint64_t)part[5 * b + 4];
    }
    return GS_OK;
}

// Everything that described the old storage layout goes back to its state at creation: a pending projection, the last draw, the
// statistics, the draw feedback words and the per-set visibility masks.  No work of the mesh is in flight.
static void mesh_forget_layout(gs_mesh* m) {
    m->layout_version++;
    m->projection_pending = false;
    m->has_draw = false;
    m->last_count = 0;
    m->last = gs_render_stats();
    m->last_pp = ProjectParams();
    m->stats_of = StatsOf();
    m->plan = SchedulePlan();
    m->list_shift = m->drawn_list_shift = GS_LIST_SHIFT_LARGE;
    m->measured_visible = m->measured_count = 0;
    m->draw_serial = m->healed_serial = m->adapted_serial = 0;
    m->grow_entries_to = 0;
    m->truncated_draws = 0;
    for (int k = 0; k < 8; k++) m->full_serial[k] = m->full_count[k] = 0;
    memset(m->mirror_host, 0, 64);                          // the draw feedback words (no draw is in flight)
    m->cur_set = 0;
    for (ProjSet& ps : m->sets) {
        ps.drawn = false;
        ps.vis_orig_lazy = false; ps.vis_orig_dirty = true; ps.vis_orig_tail_zero = false; ps.vis_orig_count = 0;
    }
}

extern "C" int gs_mesh_remove(gs_mesh* m, const uint32_t* ranges, uint32_t n_ranges, const uint32_t* scene_remap, uint32_t scene_remap_count) {
    GS_REQUIRE(m != nullptr, "mesh == NULL");
    if (n_ranges == 0) return GS_OK;
    GS_REQUIRE(ranges != nullptr, "ranges == NULL");
    GS_REQUIRE(n_ranges <= GS_MAX_SCENES, "gs_mesh_remove: more than GS_MAX_SCENES ranges");
    GS_REQUIRE(scene_remap || scene_remap_count == 0, "gs_mesh_remove: scene_remap == NULL with a count");
    GS_REQUIRE(scene_remap_count <= GS_MAX_SCENES, "gs_mesh_remove: scene_remap_count > GS_MAX_SCENES");
    for (uint32_t k = 0; k < scene_remap_count; k++) GS_REQUIRE(scene_remap[k] < GS_MAX_SCENES, "gs_mesh_remove: scene_remap entry >= GS_MAX_SCENES");
    const RemovePlan plan = plan_remove(m->runs, m->slotted, m->uploaded, m->max_count, m->reorder, ranges, n_ranges);
    if (plan.refused) {
        gs_set_error("invalid argument: gs_mesh_remove: %s", plan.refused);
        return GS_ERR_INVALID;
    }
    if (plan.removed == 0) return GS_OK;                    // every range lies beyond the uploaded splats
    gs_context* ctx = m->ctx;
    ScopedDevice sd(ctx->device);
    hipStream_t st = ctx->stream;
    // draws in flight read the planes and the permutation on either stream, a bound sorter's sort reads the permutation on its own
    GS_HIP(hipStreamSynchronize(st));
    if (ctx->aux != st) GS_HIP(hipStreamSynchronize(ctx->aux));
    for (gs_sorter* s : ctx->live_sorters)
        if ((s->bound_mesh == m || s->result_mesh == m) && s->stream != st) GS_HIP(hipStreamSynchronize(s->stream));

    const uint32_t old_end = m->uploaded, new_end = plan.uploaded;
    const uint32_t base = plan.cuts[0].begin & ~3u;         // a multiple of every plane's elements per 16 bytes; <= new_end
    GS_TRY(m->staging.ensure((size_t)(new_end - base) * 16 + 16));
    const RemoveMap map = gs_remove_map(plan, scene_remap, scene_remap_count);
    const bool half = (m->flags & GS_MESH_COV_HALF) != 0, sh_u8 = (m->flags & GS_MESH_SH_U8) != 0;
    struct Plane { DevBuf* buf; uint32_t bytes; int mode; };
    const Plane planes[] = {
        {&m->px, 4, GS_REMOVE_PLAIN}, {&m->py, 4, GS_REMOVE_PLAIN}, {&m->pz, 4, GS_REMOVE_PLAIN},
        {&m->covA, half ? 8u : 16u, GS_REMOVE_PLAIN}, {&m->covB, half ? 4u : 8u, GS_REMOVE_PLAIN},
        {&m->cov_bound, 4, GS_REMOVE_PLAIN}, {&m->rgba, 4, GS_REMOVE_PLAIN},
        {&m->sh0, 16, GS_REMOVE_PLAIN}, {&m->sh1, sh_u8 ? 8u : (m->sh_degree == 2 ? 16u : 4u), GS_REMOVE_PLAIN}, {&m->sh2, 16, GS_REMOVE_PLAIN},
        {&m->scene_idx, 4, GS_REMOVE_SCENES}, {&m->perm, 4, GS_REMOVE_POSITIONS}, {&m->inv_perm, 4, GS_REMOVE_POSITIONS},
    };
    for (const Plane& p : planes)
        GS_TRY(gs_remove_compact(st, map, p.buf->p, p.bytes, p.mode, base, new_end, old_end, m->staging.p));
    if (m->reorder) {                                       // the tail is the identity again, as gs_mesh_create left it
        hipLaunchKernelGGL(k_remove_iota, dim3(edit_grid(old_end - new_end)), dim3(256), 0, st, m->perm.as<uint32_t>(), m->inv_perm.as<uint32_t>(),
                           new_end, old_end);
        GS_HIP(hipGetLastError());
    }
    // the boxes of every storage block from the first one that changed to the old end (the blocks behind the new end: the origin)
    GS_TRY(gs_mesh_block_boxes(m, plan.first_block, (old_end + UPLOAD_BLOCK - 1u) / UPLOAD_BLOCK));
    GS_HIP(hipStreamSynchronize(st));

    // the numbering changed
    m->slotted = plan.slotted;
    m->runs = plan.runs;
    m->uploaded = new_end;
    mesh_forget_layout(m);
    GS_TRY(mesh_recount_centres(m));                       // a heuristic's inputs: the sums of the survivors
    for (gs_sorter* s : ctx->live_sorters)
        if (s->bound_mesh == m || s->result_mesh == m) gs_sorter_mesh_edited(s);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// Changing the capacity (gs_mesh_resize; gs_sorter_resize in sorter.hip).  The object moves from its capacity
// list at one capacity to the list at another (gs_internal.hpp, CapBuf): the scratch goes first - it holds nothing that outlives a
// draw or a sort - then every buffer of the new list is allocated before a resident one of the old list is released, so a failed
// allocation leaves the splats where they are.  Plain device-to-device copies move the uploaded positions.
// ---------------------------------------------------------------------------------------------------
int gs_capacity_move(hipStream_t st, const std::vector<CapBuf>& now, const std::vector<CapBuf>& next, uint32_t uploaded) {
    const size_t count = next.size();
    auto resident = [](const CapBuf& c) { return c.role == CAP_PLANE || c.role == CAP_POSITIONS || c.role == CAP_BOXES; };
    for (const CapBuf& c : now)
        if (!resident(c)) c.buf->release();
    std::vector<DevBuf> fresh(count);                       // the resident buffers at the new capacity
    int status = GS_OK;
    for (size_t k = 0; k < count && status == GS_OK; k++) {
        if (resident(next[k])) status = fresh[k].alloc(next[k].bytes);
        else if (next[k].role == CAP_SCRATCH) status = next[k].buf->alloc(next[k].bytes);
    }
    if (status != GS_OK) {
        // Back to the present capacity.  Memory ran out, so first everything this call allocated goes - the new resident planes
        // and the scratch of the new list - and only then is the scratch allocated as it was sized before: the recovery holds no
        // more than the object held when it was called.  Should even that fail (somebody else took the memory meanwhile), the
        // object is left without scratch and the caller marks it (GS_CAPACITY_SCRATCH_LOST -> scratch_lost): draws, sorts and
        // uploads are refused, never run on null buffers, until a resize succeeds.
        fresh.clear();
        for (const CapBuf& c : next)
            if (c.role == CAP_SCRATCH) c.buf->release();
        for (const CapBuf& c : now)
            if (c.role == CAP_SCRATCH && c.buf->alloc(c.bytes) != GS_OK) {
                for (const CapBuf& d : now)
                    if (d.role == CAP_SCRATCH) d.buf->release();
                return GS_CAPACITY_SCRATCH_LOST;
            }
        return status;
    }
    // (a failing copy below is a sticky HIP error: the context is lost with it, whatever capacity the object then reports)
    for (size_t k = 0; k < count; k++) {
        const CapBuf& c = next[k];
        if (!resident(c)) continue;
        // positions (CAP_BOXES: storage blocks) that hold something, then what a fresh object holds behind them
        const size_t keep = (c.role == CAP_BOXES ? ((size_t)uploaded + UPLOAD_BLOCK - 1u) / UPLOAD_BLOCK : (size_t)uploaded) * c.elem;
        if (keep) GS_HIP(hipMemcpyAsync(fresh[k].p, c.buf->p, keep, hipMemcpyDeviceToDevice, st));
        if (c.role != CAP_POSITIONS && fresh[k].bytes > keep)
            GS_HIP(hipMemsetAsync(static_cast<char*>(fresh[k].p) + keep, 0, fresh[k].bytes - keep, st));
    }
    GS_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < count; k++)
        if (resident(next[k])) next[k].buf->swap(fresh[k]);   // (the old planes go with `fresh`)
    return GS_OK;
}

extern "C" int gs_mesh_resize(gs_mesh* m, uint32_t max_splat_count) {
    GS_REQUIRE(m != nullptr, "mesh == NULL");
    if (max_splat_count == m->max_count && !m->scratch_lost) return GS_OK;
    GS_REQUIRE(max_splat_count > 0, "gs_mesh_resize: max_splat_count == 0");
    GS_REQUIRE(max_splat_count <= (1u << 28), "gs_mesh_resize: max_splat_count > 2^28");
    if (max_splat_count < m->uploaded) {
        gs_set_error("invalid argument: gs_mesh_resize: max_splat_count %u is below the uploaded count %u (remove splats first)", max_splat_count,
                     m->uploaded);
        return GS_ERR_INVALID;
    }
    gs_context* ctx = m->ctx;
    ScopedDevice sd(ctx->device);
    hipStream_t st = ctx->stream;
    // draws in flight read the planes and the permutation on either stream, a bound sorter's sort reads the permutation on its own
    GS_HIP(hipStreamSynchronize(st));
    if (ctx->aux != st) GS_HIP(hipStreamSynchronize(ctx->aux));
    for (gs_sorter* s : ctx->live_sorters)
        if ((s->bound_mesh == m || s->result_mesh == m) && s->stream != st) GS_HIP(hipStreamSynchronize(s->stream));

    // whatever comes of it, the per-frame buffers go: nothing that described a draw or a projection is left
    mesh_forget_layout(m);
    for (gs_sorter* s : ctx->live_sorters)
        if (s->bound_mesh == m || s->result_mesh == m) gs_sorter_mesh_edited(s);
    const int moved = gs_capacity_move(st, gs_mesh_capacity_list(m, m->max_count), gs_mesh_capacity_list(m, max_splat_count), m->uploaded);
    m->scratch_lost = moved == GS_CAPACITY_SCRATCH_LOST;
    if (moved != GS_OK) return m->scratch_lost ? GS_ERR_NOMEM : moved;
    m->max_count = max_splat_count;
    m->entry_capacity = std::max(m->entry_capacity, gs_mesh_entry_guess(max_splat_count));   // (the list's ekey / eval buffers)
    if (m->reorder && max_splat_count > m->uploaded) {      // the tail is the identity, as gs_mesh_create leaves it
        hipLaunchKernelGGL(k_remove_iota, dim3(edit_grid(max_splat_count - m->uploaded)), dim3(256), 0, st, m->perm.as<uint32_t>(),
                           m->inv_perm.as<uint32_t>(), m->uploaded, max_splat_count);
        GS_HIP(hipGetLastError());
    }
    // the box of the partial block at the end of the uploaded splats: it sees the zeros up to the new capacity, as a fresh mesh's does
    GS_TRY(gs_mesh_block_boxes(m, m->uploaded / UPLOAD_BLOCK, (m->uploaded + UPLOAD_BLOCK - 1u) / UPLOAD_BLOCK));
    GS_HIP(hipStreamSynchronize(st));
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// Folding the Morton runs of a range into one (gs_mesh_reorder).  The range keeps its storage slots; inside them
// the splats take the order one upload of the range would have given them.  The order itself is mesh.hip's (gs_mesh_morton_sort),
// fed with the centres as an upload stages them: in original index order, out of the planes.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reorder_centres(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz,
                                                         const uint32_t* __restrict__ perm, uint32_t from, uint32_t count,
                                                         float* __restrict__ c3) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const uint32_t s = perm[from + i];                  // (inside [from, from + count): the range is the union of its runs)
        c3[3 * (size_t)i] = px[s];
        c3[3 * (size_t)i + 1] = py[s];
        c3[3 * (size_t)i + 2] = pz[s];
    }
}

// source[p] = where, counted from `from`, the splat of the NEW storage position from + p lies now (read before perm is rewritten)
__global__ __launch_bounds__(256) void k_reorder_source(const uint32_t* __restrict__ sorted_local, const uint32_t* __restrict__ perm, uint32_t from,
                                                        uint32_t count, uint32_t* __restrict__ source) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < count; p += gridDim.x * blockDim.x) {
        const uint32_t s = perm[from + sorted_local[p]] - from;
        source[p] = s < count ? s : count - 1u;             // (inside the range by the run rule; were it ever not, the move reads no wild address)
    }
}

// The move of one plane group: up to 16 bytes per splat, planes of one element size, so that a position's source index is read
// once for all of them.  The reads are scattered by nature (the old order is the trainer's); the writes are in order.
constexpr uint32_t REORDER_GROUP_BYTES = 16;
template <class T>
struct ReorderGroup {
    T* plane[REORDER_GROUP_BYTES / sizeof(T)];              // the planes' first elements
    uint32_t n;
};
template <class T>
__global__ __launch_bounds__(256) void k_reorder_move(ReorderGroup<T> g, const T* __restrict__ scratch, uint32_t stride,
                                                      const uint32_t* __restrict__ source, uint32_t from, uint32_t count) {
    constexpr uint32_t MAXP = REORDER_GROUP_BYTES / sizeof(T);
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < count; p += gridDim.x * blockDim.x) {
        const uint32_t s = source[p];
        T v[MAXP];
#pragma unroll
        for (uint32_t k = 0; k < MAXP; k++)
            if (k < g.n) v[k] = scratch[(size_t)k * stride + s];
#pragma unroll
        for (uint32_t k = 0; k < MAXP; k++)
            if (k < g.n) g.plane[k][from + p] = v[k];
    }
}

// copies the range of every plane of the group into the scratch (one behind the other, `stride` elements apart), then gathers back
template <class T>
static int reorder_group(hipStream_t st, const ReorderGroup<T>& g, void* scratch, uint32_t stride, const uint32_t* source, uint32_t from,
                         uint32_t count) {
    for (uint32_t k = 0; k < g.n; k++)
        GS_HIP(hipMemcpyAsync(static_cast<T*>(scratch) + (size_t)k * stride, g.plane[k] + from, (size_t)count * sizeof(T), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_reorder_move<T>, dim3(edit_grid(count)), dim3(256), 0, st, g, (const T*)scratch, stride, source, from, count);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// every plane of `bytes`-sized elements among planes[0 .. n), a group at a time
template <class T>
static int reorder_planes_of(hipStream_t st, void* const* planes, const uint32_t* bytes, uint32_t n, void* scratch, uint32_t stride,
                             const uint32_t* source, uint32_t from, uint32_t count) {
    ReorderGroup<T> g = {};
    for (uint32_t k = 0; k < n; k++) {
        if (!planes[k] || bytes[k] != sizeof(T)) continue;
        g.plane[g.n++] = static_cast<T*>(planes[k]);
        if (g.n == REORDER_GROUP_BYTES / sizeof(T)) {
            GS_TRY(reorder_group(st, g, scratch, stride, source, from, count));
            g.n = 0;
        }
    }
    if (g.n) GS_TRY(reorder_group(st, g, scratch, stride, source, from, count));
    return GS_OK;
}

extern "C" int gs_mesh_reorder(gs_mesh* m, uint32_t from, uint32_t count) {
    GS_REQUIRE(m != nullptr, "mesh == NULL");
    GS_REQUIRE_SCRATCH(m);
    const ReorderPlan plan = plan_reorder(m->runs, m->slotted, m->uploaded, m->reorder, from, count);
    if (plan.refused) {
        gs_set_error("invalid argument: gs_mesh_reorder: %s", plan.refused);
        return GS_ERR_INVALID;
    }
    if (plan.noop) return GS_OK;
    gs_context* ctx = m->ctx;
    ScopedDevice sd(ctx->device);
    hipStream_t st = ctx->stream;
    // draws in flight read the planes and the permutation on either stream, a bound sorter's sort reads the permutation on its own
    GS_HIP(hipStreamSynchronize(st));
    if (ctx->aux != st) GS_HIP(hipStreamSynchronize(ctx->aux));
    for (gs_sorter* s : ctx->live_sorters)
        if ((s->bound_mesh == m || s->result_mesh == m) && s->stream != st) GS_HIP(hipStreamSynchronize(s->stream));

    // the scratch: first the centres float [3n], then one plane group (stride: whole 16-byte units per plane)
    const uint32_t stride16 = (count + 3u) & ~3u;
    GS_TRY(m->staging.ensure((size_t)stride16 * REORDER_GROUP_BYTES));
    float* c3 = m->staging.as<float>();
    hipLaunchKernelGGL(k_reorder_centres, dim3(edit_grid(count)), dim3(256), 0, st, m->px.as<float>(), m->py.as<float>(), m->pz.as<float>(),
                       m->perm.as<uint32_t>(), from, count, c3);
    GS_HIP(hipGetLastError());
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    GS_TRY(gs_mesh_centre_bounds(m, c3, count, mn, mx, false));   // the centre sums stay: the fold moves splats, it changes none
    const uint32_t* sorted_local = nullptr;
    uint32_t* source = nullptr;
    GS_TRY(gs_mesh_morton_sort(m, c3, count, mn, mx, &sorted_local, &source));
    hipLaunchKernelGGL(k_reorder_source, dim3(edit_grid(count)), dim3(256), 0, st, sorted_local, m->perm.as<uint32_t>(), from, count, source);
    GS_HIP(hipGetLastError());
    GS_TRY(gs_mesh_assign_slots(m, sorted_local, from, count));

    // every per-splat plane kept in storage order (gs_mesh_remove's list; perm and inv_perm are rewritten above)
    const bool half = (m->flags & GS_MESH_COV_HALF) != 0, sh_u8 = (m->flags & GS_MESH_SH_U8) != 0;
    void* const planes[] = {m->px.p, m->py.p, m->pz.p, m->cov_bound.p, m->rgba.p, m->scene_idx.p, m->covA.p, m->covB.p, m->sh0.p, m->sh1.p, m->sh2.p};
    const uint32_t bytes[] = {4, 4, 4, 4, 4, 4, half ? 8u : 16u, half ? 4u : 8u, 16, sh_u8 ? 8u : (m->sh_degree == 2 ? 16u : 4u), 16};
    constexpr uint32_t N = sizeof(bytes) / sizeof(bytes[0]);
    GS_TRY(reorder_planes_of<uint32_t>(st, planes, bytes, N, m->staging.p, stride16, source, from, count));
    GS_TRY(reorder_planes_of<uint2>(st, planes, bytes, N, m->staging.p, stride16, source, from, count));
    GS_TRY(reorder_planes_of<uint4>(st, planes, bytes, N, m->staging.p, stride16, source, from, count));
    GS_TRY(gs_mesh_block_boxes(m, plan.first_block, plan.end_block));
    GS_HIP(hipStreamSynchronize(st));

    m->runs = plan.runs;
    mesh_forget_layout(m);
    for (gs_sorter* s : ctx->live_sorters)
        if (s->bound_mesh == m || s->result_mesh == m) gs_sorter_mesh_reordered(s);
    return GS_OK;
}
