// extreme_set.cpp — see extreme_set.hpp.  An iterated inner-polytope filter:
//   1. the extreme points of the input in 26 fixed directions span a first polytope H (an incremental convex hull with exact
//      __int128 orientation tests; its vertices are input points);
//   2. every point strictly inside H is dropped (doubles + a margin that can only keep; first a ball inscribed in H);
//   3. for every facet of H the survivor farthest outside it joins H; back to 2 until the survivors fit the cap.
// The survivors are the set: nothing else is ever dropped, so every hull vertex of the input is among them.  Inputs that lie in one
// plane, on one line or in one point have no polytope with an inside: their exact 2-D hull / two ends / one point are the set.
// All coordinates are int32: differences fit 33 bits, a normal's components 67, an orientation 101 - exact in __int128.
#include "extreme_set.hpp"

#include <math.h>

#include <algorithm>
#include <new>
#include <utility>

namespace {

typedef __int128 i128;

struct P { int32_t x, y, z; };
inline bool operator==(const P& a, const P& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
inline bool lex_less(const P& a, const P& b) { return a.x != b.x ? a.x < b.x : (a.y != b.y ? a.y < b.y : a.z < b.z); }
struct D3 { int64_t x, y, z; };
inline D3 sub(const P& a, const P& b) { return {(int64_t)a.x - b.x, (int64_t)a.y - b.y, (int64_t)a.z - b.z}; }
struct N3 { i128 x, y, z; };
inline N3 cross(const D3& u, const D3& v) {
    return {(i128)u.y * v.z - (i128)u.z * v.y, (i128)u.z * v.x - (i128)u.x * v.z, (i128)u.x * v.y - (i128)u.y * v.x};
}
inline i128 dot(const N3& n, const D3& d) { return n.x * d.x + n.y * d.y + n.z * d.z; }
inline bool is_zero(const N3& n) { return n.x == 0 && n.y == 0 && n.z == 0; }
inline double len2(const N3& n) { return (double)n.x * (double)n.x + (double)n.y * (double)n.y + (double)n.z * (double)n.z; }
inline double dabs128(i128 v) { return fabs((double)v); }

// the input: two AoS x4 arrays, one after the other
struct Src {
    const int32_t* a; size_t na;
    const int32_t* b; size_t nb;
    size_t size() const { return na + nb; }
    P at(size_t i) const {
        const int32_t* r = i < na ? a + 4 * i : b + 4 * (i - na);
        return {r[0], r[1], r[2]};
    }
};

// relative margin of n . (q - a) in doubles: the normal's components are rounded once (2^-53 each), the differences are exact,
// three products and two sums round once each - below 2^-50 of |t0| + |t1| + |t2|; 2^-45 leaves a factor of 32
constexpr double FILTER_EPS = 1.0 / 35184372088832.0;

// ---------------------------------------------------------------------------------------------------
// incremental hull of a few points, exact.  Faces are triangles with outward normals; a point joins when it is STRICTLY outside
// some face's plane (the faces it sees are removed, the horizon is joined to it).  A point in the closed polytope sees nothing and
// is ignored, so what the faces bound is always the convex hull of `vert`, and vert holds input points only.
// ---------------------------------------------------------------------------------------------------
struct Face { uint32_t v[3]; N3 n; double dn[3]; bool alive; };   // dn: the normal in doubles (a first look before the exact test)
struct Hull {
    std::vector<P> vert;
    std::vector<Face> faces;
    size_t alive = 0;
    std::vector<uint32_t> vis;
    std::vector<uint64_t> edges;

    void add_face(uint32_t a, uint32_t b, uint32_t c) {
        Face f;
        f.v[0] = a; f.v[1] = b; f.v[2] = c;
        f.n = cross(sub(vert[b], vert[a]), sub(vert[c], vert[a]));
        f.dn[0] = (double)f.n.x; f.dn[1] = (double)f.n.y; f.dn[2] = (double)f.n.z;
        f.alive = true;
        faces.push_back(f);
        alive++;
    }
    void add_face_away_from(uint32_t a, uint32_t b, uint32_t c, uint32_t opp) {
        const N3 n = cross(sub(vert[b], vert[a]), sub(vert[c], vert[a]));
        if (dot(n, sub(vert[opp], vert[a])) > 0) std::swap(b, c);
        add_face(a, b, c);
    }
    void init(const P& a, const P& b, const P& c, const P& d) {       // four points that are not in one plane
        vert = {a, b, c, d};
        add_face_away_from(0, 1, 2, 3);
        add_face_away_from(0, 1, 3, 2);
        add_face_away_from(0, 2, 3, 1);
        add_face_away_from(1, 2, 3, 0);
    }
    // p strictly outside face f's plane: doubles decide what lies clear of their own error (FILTER_EPS), __int128 the rest
    bool sees(const Face& f, const P& p) const {
        const D3 d = sub(p, vert[f.v[0]]);
        const double t0 = f.dn[0] * (double)d.x, t1 = f.dn[1] * (double)d.y, t2 = f.dn[2] * (double)d.z;
        const double val = t0 + t1 + t2, mar = (fabs(t0) + fabs(t1) + fabs(t2)) * FILTER_EPS;
        if (val > mar) return true;
        if (val < -mar) return false;
        return dot(f.n, d) > 0;
    }
    bool insert(const P& p) {
        vis.clear();
        for (uint32_t f = 0; f < faces.size(); f++)
            if (faces[f].alive && sees(faces[f], p)) vis.push_back(f);
        if (vis.empty()) return false;
        edges.clear();
        for (uint32_t f : vis)
            for (int k = 0; k < 3; k++) edges.push_back((uint64_t)faces[f].v[k] << 32 | faces[f].v[(k + 1) % 3]);
        std::sort(edges.begin(), edges.end());
        const uint32_t pi = (uint32_t)vert.size();
        vert.push_back(p);
        for (uint32_t f : vis) faces[f].alive = false;
        alive -= vis.size();
        const size_t ne = edges.size();
        for (size_t e = 0; e < ne; e++) {                              // a horizon edge: its reverse belongs to a face p does not see
            const uint32_t u = (uint32_t)(edges[e] >> 32), v = (uint32_t)edges[e];
            if (!std::binary_search(edges.begin(), edges.begin() + ne, (uint64_t)v << 32 | u)) add_face(u, v, pi);
        }
        if (faces.size() > 64 && alive * 2 < faces.size()) {
            size_t w = 0;
            for (size_t f = 0; f < faces.size(); f++)
                if (faces[f].alive) faces[w++] = faces[f];
            faces.resize(w);
        }
        return true;
    }
};

// a face for the bulk filter
struct FaceD { double nx, ny, nz, ax, ay, az, inv_len; };


struct Filter {
    std::vector<FaceD> fd;
    std::vector<double> best;
    std::vector<P> best_p;
    double cx = 0, cy = 0, cz = 0, r2 = -1.0;
    double work = 0;

    void prepare(const Hull& h) {
        fd.clear();
        for (const Face& f : h.faces) {
            if (!f.alive) continue;
            FaceD d;
            d.nx = (double)f.n.x; d.ny = (double)f.n.y; d.nz = (double)f.n.z;
            const P& a = h.vert[f.v[0]];
            d.ax = a.x; d.ay = a.y; d.az = a.z;
            const double l = sqrt(d.nx * d.nx + d.ny * d.ny + d.nz * d.nz);
            d.inv_len = l > 0 ? 1.0 / l : 0.0;
            fd.push_back(d);
        }
        best.assign(fd.size(), 0.0);
        best_p.assign(fd.size(), P{0, 0, 0});
        // a ball inside H about the mean of its vertices (inside H, or on its boundary when H is flat there: then r = 0, no ball)
        cx = cy = cz = 0;
        for (const P& v : h.vert) { cx += v.x; cy += v.y; cz += v.z; }
        cx /= (double)h.vert.size(); cy /= (double)h.vert.size(); cz /= (double)h.vert.size();
        double r = INFINITY;
        for (const FaceD& d : fd) r = fmin(r, -(d.nx * (cx - d.ax) + d.ny * (cy - d.ay) + d.nz * (cz - d.az)) * d.inv_len);
        r *= 1.0 - 1e-6;                                               // (the errors above are ~1e-15 of r)
        r2 = (r > 0 && r < INFINITY) ? r * r : -1.0;
    }
    // true: q is kept (not proven strictly inside H)
    bool keep(const P& q) {
        const double dx = q.x - cx, dy = q.y - cy, dz = q.z - cz;
        if (dx * dx + dy * dy + dz * dz < r2) return false;
        const size_t nf = fd.size();
        for (size_t f = 0; f < nf; f++) {
            const FaceD& d = fd[f];
            const double t0 = d.nx * (q.x - d.ax), t1 = d.ny * (q.y - d.ay), t2 = d.nz * (q.z - d.az);
            const double val = t0 + t1 + t2;
            if (val >= -(fabs(t0) + fabs(t1) + fabs(t2)) * FILTER_EPS) {      // not strictly inside this face's plane
                const double dist = val * d.inv_len;
                if (dist > best[f]) { best[f] = dist; best_p[f] = q; }
                work += (double)(f + 1);
                return true;
            }
        }
        work += (double)nf;
        return false;
    }
};

void emit(const std::vector<P>& s, std::vector<int32_t>& out) {
    out.clear();
    out.reserve(s.size() * 4);
    for (const P& p : s) { out.push_back(p.x); out.push_back(p.y); out.push_back(p.z); out.push_back(0); }
}

void dedupe(std::vector<P>& s) {
    std::sort(s.begin(), s.end(), lex_less);
    s.erase(std::unique(s.begin(), s.end()), s.end());
}

// every input point lies in the plane through p0 with normal n: the vertices of the exact 2-D hull (monotone chain in the two
// coordinates that are left when the normal's largest component is dropped - an affine bijection of the plane)
void planar_hull(const Src& src, const N3& n, std::vector<P>& out) {
    const double ax = dabs128(n.x), ay = dabs128(n.y), az = dabs128(n.z);
    const int drop = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    struct Q { int64_t u, v; P p; };
    std::vector<Q> q(src.size());
    for (size_t i = 0; i < src.size(); i++) {
        const P p = src.at(i);
        q[i].p = p;
        q[i].u = drop == 0 ? p.y : p.x;
        q[i].v = drop == 2 ? p.y : p.z;
    }
    std::sort(q.begin(), q.end(), [](const Q& a, const Q& b) { return a.u != b.u ? a.u < b.u : a.v < b.v; });
    q.erase(std::unique(q.begin(), q.end(), [](const Q& a, const Q& b) { return a.u == b.u && a.v == b.v; }), q.end());
    auto turn = [](const Q& o, const Q& a, const Q& b) { return (i128)(a.u - o.u) * (b.v - o.v) - (i128)(a.v - o.v) * (b.u - o.u); };
    std::vector<Q> h;
    const size_t m = q.size();
    for (size_t i = 0; i < m; i++) {                                   // lower chain
        while (h.size() >= 2 && turn(h[h.size() - 2], h[h.size() - 1], q[i]) <= 0) h.pop_back();
        h.push_back(q[i]);
    }
    const size_t lower = h.size() + 1;
    for (size_t i = m - 1; i-- > 0;) {                                 // upper chain
        while (h.size() >= lower && turn(h[h.size() - 2], h[h.size() - 1], q[i]) <= 0) h.pop_back();
        h.push_back(q[i]);
    }
    if (h.size() > 1) h.pop_back();
    out.clear();
    for (const Q& e : h) out.push_back(e.p);
}

// a point with a non-zero cross product against p0 -> p1, the largest (in doubles: any non-zero one serves)
template <class At>
bool find_off_line(size_t n, At at, const P& p0, const P& p1, P& p2) {
    double best = 0;
    const D3 u = sub(p1, p0);
    for (size_t i = 0; i < n; i++) {
        const P q = at(i);
        const N3 c = cross(u, sub(q, p0));
        if (is_zero(c)) continue;
        const double l = len2(c);                                      // (>= 1 for a non-zero integer vector)
        if (l > best) { best = l; p2 = q; }
    }
    return best > 0;
}
template <class At>
bool find_off_plane(size_t n, At at, const P& p0, const N3& nrm, P& p3) {
    double best = 0;
    for (size_t i = 0; i < n; i++) {
        const P q = at(i);
        const i128 o = dot(nrm, sub(q, p0));
        if (o == 0) continue;
        const double l = dabs128(o);
        if (l > best) { best = l; p3 = q; }
    }
    return best > 0;
}

bool build(const Src& src, uint32_t cap, std::vector<P>& out) {
    const size_t n = src.size();
    out.clear();
    if (n == 0) return true;
    // 1. extreme points in the 26 directions of {-1, 0, 1}^3, and the lexicographic ends
    int dir[26][3];
    int nd = 0;
    for (int a = -1; a <= 1; a++)
        for (int b = -1; b <= 1; b++)
            for (int c = -1; c <= 1; c++)
                if (a || b || c) { dir[nd][0] = a; dir[nd][1] = b; dir[nd][2] = c; nd++; }
    int64_t best[26];
    P ext[28];
    P p0 = src.at(0), p1 = p0;
    for (int d = 0; d < 26; d++) { best[d] = INT64_MIN; ext[d] = p0; }
    for (size_t i = 0; i < n; i++) {
        const P q = src.at(i);
        if (lex_less(q, p0)) p0 = q;
        if (lex_less(p1, q)) p1 = q;
        for (int d = 0; d < 26; d++) {
            const int64_t v = (int64_t)dir[d][0] * q.x + (int64_t)dir[d][1] * q.y + (int64_t)dir[d][2] * q.z;
            if (v > best[d]) { best[d] = v; ext[d] = q; }
        }
    }
    ext[26] = p0; ext[27] = p1;
    if (p0 == p1) {                                                    // one point
        out.push_back(p0);
        return true;
    }
    // 2. four points that span space: among the extreme points, else among all
    auto at_ext = [&](size_t i) { return ext[i]; };
    auto at_all = [&](size_t i) { return src.at(i); };
    P p2 = p0, p3 = p0;
    if (!find_off_line(28, at_ext, p0, p1, p2) && !find_off_line(n, at_all, p0, p1, p2)) {
        out.push_back(p0);                                             // one line: its two ends
        out.push_back(p1);
        return true;
    }
    const N3 nrm = cross(sub(p1, p0), sub(p2, p0));
    if (!find_off_plane(28, at_ext, p0, nrm, p3) && !find_off_plane(n, at_all, p0, nrm, p3)) {
        planar_hull(src, nrm, out);                                    // one plane
        if (out.size() > cap) { out.clear(); return false; }
        return true;
    }
    Hull h;
    h.init(p0, p1, p2, p3);
    for (int d = 0; d < 28; d++) h.insert(ext[d]);

    // 3. filter, grow H by the farthest survivor outside each facet, filter again
    Filter flt;
    std::vector<P> s;
    size_t prev = n;
    bool reached = false;
    const double budget = 2.0e9;                                       // face tests in all: bounds the set-up time of a hopeless scene
    for (int round = 0; round < 48; round++) {
        flt.prepare(h);
        if (round == 0) {
            for (size_t i = 0; i < n; i++) {
                const P q = src.at(i);
                if (flt.keep(q)) s.push_back(q);
            }
        } else {
            size_t w = 0;
            for (size_t i = 0; i < s.size(); i++)
                if (flt.keep(s[i])) s[w++] = s[i];
            s.resize(w);
        }
        if (s.size() <= ((size_t)1 << 21)) dedupe(s);
        const size_t now = s.size();
        if (now <= cap) {
            if (reached && now * 20 > prev * 19) break;                // fits, and another round no longer pays
            reached = true;
        } else {
            if (h.vert.size() > cap || flt.work > budget) break;       // more than cap hull vertices / out of budget
            if (round >= 1 && now > (size_t)64 * cap && now * 10 > prev * 7) break;   // far off and hardly shrinking (a shell)
            if (round >= 2 && now * 100 > prev * 97) break;            // H doubles every round and next to nothing falls inside it
        }
        prev = now;
        size_t joined = 0;
        for (size_t f = 0; f < flt.best.size(); f++)
            if (flt.best[f] > 0 && h.insert(flt.best_p[f])) joined++;
        if (!joined) break;                                            // H holds every survivor: nothing more can be dropped
    }
    if (s.size() > cap) return false;
    dedupe(s);
    out.swap(s);
    return true;
}

}  // namespace

bool gs_extreme_set(const int32_t* a, size_t na, const int32_t* b, size_t nb, uint32_t cap, std::vector<int32_t>& out) {
    out.clear();
    try {
        std::vector<P> s;
        const Src src = {a, na, b, nb};
        if (!build(src, cap, s)) return false;
        emit(s, out);
        return true;
    } catch (const std::bad_alloc&) {
        out.clear();
        return false;
    }
}

bool gs_compact_offsets(const int32_t* set_aos4, size_t n, int32_t offset[3]) {
    if (!set_aos4 || n == 0) return false;
    int32_t lo[3], hi[3];
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = set_aos4[k];
    for (size_t i = 1; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const int32_t v = set_aos4[4 * i + k];
            lo[k] = std::min(lo[k], v);
            hi[k] = std::max(hi[k], v);
        }
    for (int k = 0; k < 3; k++)
        if ((int64_t)hi[k] - (int64_t)lo[k] > 65535) return false;     // (int64: hi - lo reaches 2^32 - 1)
    for (int k = 0; k < 3; k++) offset[k] = lo[k];
    return true;
}

extern "C" int gs_debug_compact_offsets(const int32_t* set_aos4, uint32_t count, int32_t* offset3) {
    if (!offset3 || (count && !set_aos4)) return -1;
    return gs_compact_offsets(set_aos4, count, offset3) ? 1 : 0;
}

bool gs_key_range(const int32_t* set_aos4, size_t n, const int32_t im[3], int32_t* lo_out, int32_t* hi_out) {
    if (!set_aos4 || n == 0) return false;
    const int32_t* c = set_aos4;
    const int64_t a0 = im[0], a1 = im[1], a2 = im[2];
    const int64_t small = (int64_t)1 << 29;                // |im| <= 2^29: three products of at most 2^60 add up in int64
    __int128 lo, hi;
    if (a0 >= -small && a0 <= small && a1 >= -small && a1 <= small && a2 >= -small && a2 <= small) {
        int64_t l = INT64_MAX, h = INT64_MIN;
        for (size_t i = 0; i < n; i++) {
            const int64_t v = a0 * c[4 * i] + a1 * c[4 * i + 1] + a2 * c[4 * i + 2];
            l = v < l ? v : l;
            h = v > h ? v : h;
        }
        lo = l; hi = h;
    } else {
        lo = hi = (__int128)a0 * c[0] + (__int128)a1 * c[1] + (__int128)a2 * c[2];
        for (size_t i = 1; i < n; i++) {
            const __int128 v = (__int128)a0 * c[4 * i] + (__int128)a1 * c[4 * i + 1] + (__int128)a2 * c[4 * i + 2];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    if (lo < INT32_MIN || hi > INT32_MAX) return false;    // a key could wrap
    *lo_out = (int32_t)lo;
    *hi_out = (int32_t)hi;
    return true;
}

extern "C" int gs_debug_key_range(const int32_t* set_aos4, uint32_t count, const int32_t* im3, int32_t* lo_hi2) {
    if (!im3 || !lo_hi2 || (count && !set_aos4)) return -1;
    return gs_key_range(set_aos4, count, im3, &lo_hi2[0], &lo_hi2[1]) ? 1 : 0;
}

extern "C" int gs_debug_extreme_set(const int32_t* prior_aos4, uint32_t prior_count, const int32_t* aos4, uint32_t count, uint32_t cap,
                                    int32_t* out_aos4, uint32_t* out_count) {
    if (!out_aos4 || !out_count || (prior_count && !prior_aos4) || (count && !aos4)) return -1;
    *out_count = 0;
    std::vector<int32_t> out;
    if (!gs_extreme_set(prior_aos4, prior_count, aos4, count, cap, out)) return 1;
    std::copy(out.begin(), out.end(), out_aos4);
    *out_count = (uint32_t)(out.size() / 4);
    return 0;
}
