// extreme_set.hpp — the EXTREME SET of a static integer sorter's centres (extreme_set.cpp; host only, no device, no context).
//
// A static integer sort keys splat c with im . c (sorter.hip, static_key_int).  As long as no key wraps, that is an exact linear
// functional of the int32 centre, and the min / max of a linear functional over a point set are attained at vertices of its convex
// hull.  The extreme set C is a small subset of the centres that holds EVERY hull vertex: the host evaluates a sort's exact key
// range over C before it launches anything, and the key kernel histograms pass 0's digit itself (k_depth_key_hist).
//
// Contract: C is a subset of the input points; every vertex of the convex hull of the input is in C.  Extra points are harmless, a
// missing vertex is a wrong sort: a point is dropped only when it is proven to lie strictly inside a polytope whose vertices are
// other input points (exact __int128 orientation tests for the polytope, doubles with a margin that can only err towards keeping
// for the bulk filter), or - for a set that lies in one plane / on one line - when it is no vertex of the exact 2-D / 1-D hull.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr uint32_t GS_EXTREME_CAP = 4096;      // points (64 KB as AoS x4); a scene whose set does not fit has none

// The extreme set of (a U b), both AoS x4 int32 rows (x, y, z, ignored), into out (AoS x4, w = 0).  hull(old U new) =
// hull(C(old) U new), so an appended range extends a set from `a` = the old set and `b` = the new rows.  false: more than `cap`
// points could not be proven interior (or the work budget ran out) - no set, `out` is empty.
bool gs_extreme_set(const int32_t* a, size_t na, const int32_t* b, size_t nb, uint32_t cap, std::vector<int32_t>& out);

// Whether the centres fit 16-BIT OFFSET PLANES, decided from their extreme set (AoS x4 rows, `n` of them): every hull vertex is in
// the set, so the per-axis min and max of ALL centres are attained in it.  true: max - min <= 65535 on every axis (int64: centres
// sit anywhere in int32) and offset[k] = the minimum of axis k, so 0 <= c - offset <= 65535 for every centre.  false: an axis is
// wider, or the set is empty - `offset` is left alone.  The sorter then streams c - offset as uint16 planes in its known-range
// front end (sorter.hip, k_depth_key_hist<true, true>): im . c == im . offset + im . (c - offset) mod 2^32.
bool gs_compact_offsets(const int32_t* set_aos4, size_t n, int32_t offset[3]);

// Debug entry for the tests (pure host): 1 and offset3 = the offsets when the rows fit, 0 when they do not, -1 on bad arguments.
extern "C" int gs_debug_compact_offsets(const int32_t* set_aos4, uint32_t count, int32_t* offset3);

// The EXACT KEY RANGE of a sort, known before anything is launched: min / max of im . c over the extreme set (AoS x4 rows, `n` of
// them), in exact integers.  true only when neither end leaves int32 - then no key of any centre wraps, every key is its true
// value, and [lo, hi] is what the device-wide reduction would find.  false: a key could wrap, or the set is empty - lo / hi are
// left alone.  (Whether a sort may use the range at all is sort_plan.cpp's decision.)
bool gs_key_range(const int32_t* set_aos4, size_t n, const int32_t im[3], int32_t* lo, int32_t* hi);

// Debug entry for the tests (pure host): 1 and lo_hi2 = {lo, hi}, 0 when there is no range, -1 on bad arguments.
extern "C" int gs_debug_key_range(const int32_t* set_aos4, uint32_t count, const int32_t* im3, int32_t* lo_hi2);

// Debug entry for the tests (pure host).  out holds up to cap rows.  Returns 0 and *out_count = |C|, 1 when the set does not fit
// (*out_count = 0), -1 on bad arguments.
extern "C" int gs_debug_extreme_set(const int32_t* prior_aos4, uint32_t prior_count, const int32_t* aos4, uint32_t count, uint32_t cap,
                                    int32_t* out_aos4, uint32_t* out_count);
