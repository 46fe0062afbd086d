// ray_table_check.cpp -- testing hooks of the direction table (ray_table.cpp), host only: its guarantee, its hints and its certificates checked point by
// point against the reference's own search, and a signature of the whole table.  A hook builds the tree and the table of the mesh it is given and looks at
// them through the very functions the kernels call (search_device.hpp, which also compiles for the host).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

#include "ray_table.hpp"
#include "search_device.hpp"

namespace msm {

namespace {

// What every hook starts from: the mesh, checked; its tree and table; the host view of the table; the random numbers; the reference's leaf search.
struct TableUnderTest {
    const char *hook = "";
    const double *xyz = nullptr;
    const int32_t *tri = nullptr;
    int V = 0, T = 0;
    FlatOctree o;
    DevTree dt{};  // the table as the kernels' functions read it (o.rays' arrays: `o` must stay where it is)
    uint64_t rs = 0;
    std::vector<int> hits;

    // MSM_OK and the hook's `nreport` output words zeroed, or the error a hook returns for bad arguments
    int build(const char *hook_, const double *xyz_, const int32_t *tri_, int32_t V_, int32_t T_, int32_t nsamples, uint64_t seed, int64_t *report, int nreport) {
        hook = hook_, xyz = xyz_, tri = tri_, V = V_, T = T_;
        if (!xyz || !tri || !report || V <= 0 || T <= 0 || nsamples < 0) return fail(MSM_ERR_INVALID, "%s: bad arguments", hook);
        for (int64_t i = 0; i < 3 * (int64_t)T; ++i)
            if (tri[i] < 0 || tri[i] >= V) return fail(MSM_ERR_INVALID, "%s: triangle vertex id %d out of range [0,%d)", hook, tri[i], V);
        build_octree(xyz, tri, V, T, o);
        build_ray_table(xyz, tri, V, T, o);
        std::fill(report, report + nreport, (int64_t)0);
        dt.ray_G = o.rays.G;
        dt.ray_cell = o.rays.cell.data();
        dt.ray_more = o.rays.more.data();
        dt.ray_excl = o.rays.excl.data();
        dt.ray_r2lo = o.rays.r2lo, dt.ray_r2hi = o.rays.r2hi;
        rs = seed * 6364136223846793005ull + 1442695040888963407ull;
        return MSM_OK;
    }
    double rnd() {  // uniform in [0, 1)
        rs = rs * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(rs >> 11) * (1.0 / 9007199254740992.0);
    }
    V3 random_direction() {  // uniform in the unit ball, outside radius 0.1
        V3 p;
        do p = V3{2 * rnd() - 1, 2 * rnd() - 1, 2 * rnd() - 1};  // (a braced list is evaluated in order)
        while (!(norm(p) > 0.1 && norm(p) <= 1.0));
        return p;
    }
    V3 vert(int t, int k) const { return vtx(xyz, V, tri[(size_t)k * T + t]); }
    // the reference's first pass (R/octree.cpp:156-178): descend to the leaf of p, every listed triangle through the inside test; the ones that pass, in order
    const std::vector<int> &first_pass(const V3 &p) {
        int n = 0;
        while (o.node[n].x >= 0) {
            const double4 b = o.nodebox[n];
            const double mx = (b.x + (b.x + b.w)) / 2.0, my = (b.y + (b.y + b.w)) / 2.0, mz = (b.z + (b.z + b.w)) / 2.0;
            n = o.node[n].x + 4 * (!(p.x < mx)) + 2 * (!(p.y < my)) + (!(p.z < mz));
        }
        hits.clear();
        for (int e = 0; e < -o.node[n].x - 1; ++e) {
            const int t = o.leaf_tri[o.node[n].y + e];
            const V3 a = vert(t, 0), b = vert(t, 1), c = vert(t, 2);
            if (point_in_triangle(project_point(p, a, b, c), a, b, c)) hits.push_back(t);
        }
        return hits;
    }
    // the next point of msm_ray_hint_check and msm_ray_depth_check: a random direction on the radius shell, and the one triangle the reference's first pass
    // returns for it (-1: none, or several)
    int random_point(V3 &p) {
        p = scale(normalized(random_direction()), kRad);
        const std::vector<int> &h = first_pass(p);
        return h.size() == 1 ? h[0] : -1;
    }
    // A cell's candidates in the order a kernel tries them: x, y, z, then w or, where w refers to one, the four ids of the cell's ray_more entry; the first
    // negative id ends the list.  c: the cell as ray_cell_of hands it out (the hinted candidate first), or its stored ids (ray_cell_ids).
    std::array<int, 7> candidates(const int4 &c) const {
        int4 more = make_int4(c.w, -1, -1, -1);
        if (c.x >= 0 && c.w < -1) more = o.rays.more[-2 - c.w];
        return {c.x, c.y, c.z, more.x, more.y, more.z, more.w};
    }
    // the cell array as stored into cells (may be NULL: nothing to do), when cells_cap words hold it
    int copy_cells(int32_t *cells, int64_t cells_cap) const {
        const size_t ncell = o.rays.cell.size();
        if (!cells) return MSM_OK;
        if (cells_cap < 4 * (int64_t)ncell) return fail(MSM_ERR_INVALID, "%s: room for %lld words, the cells have %lld", hook, (long long)cells_cap, (long long)(4 * ncell));
        std::memcpy(cells, o.rays.cell.data(), ncell * sizeof(int4));
        return MSM_OK;
    }
};

// msm_ray_table_check's point number `it`, on the shell: a random direction, or a point next to an edge or a vertex of a random triangle, or (every fifth, when
// there are any) a point above one of the `guarded` triangles -- the ones with exclusion boxes
V3 table_check_point(TableUnderTest &u, const std::vector<int> &guarded, int it) {
    const int T = u.T;
    V3 p;
    const int kind = (it % 5 == 4 && !guarded.empty()) ? 4 : it % 4;
    if (kind == 4) {  // above a triangle with exclusion boxes, towards its rim (where the shell region leaves the triangle's own box)
        const int t = guarded[(size_t)(u.rnd() * guarded.size()) % guarded.size()];
        double w[3] = {u.rnd(), u.rnd() * 0.05, u.rnd() * 0.05};  // (a braced list is evaluated in order)
        const int k = (int)(u.rnd() * 3) % 3;
        std::swap(w[0], w[k]);
        const V3 a = u.vert(t, 0), b = u.vert(t, 1), c = u.vert(t, 2);
        p = mk(w[0] * a.x + w[1] * b.x + w[2] * c.x, w[0] * a.y + w[1] * b.y + w[2] * c.y, w[0] * a.z + w[1] * b.z + w[2] * c.z);
    } else if (kind == 0) {  // a random direction
        p = u.random_direction();
    } else {  // next to an edge (kind 1, 2) or a vertex (kind 3) of a random triangle, on either side
        const int t = (int)(u.rnd() * T) % T, k = (int)(u.rnd() * 3) % 3;
        const V3 a = u.vert(t, k), b = u.vert(t, (k + 1) % 3), c = u.vert(t, (k + 2) % 3);
        const double along = kind == 3 ? (u.rnd() < 0.5 ? 0.0 : 1e-9 * u.rnd()) : u.rnd();
        const V3 on = mk(a.x + along * (b.x - a.x), a.y + along * (b.y - a.y), a.z + along * (b.z - a.z));
        const double side = u.rnd() < 0.5 ? -1.0 : 1.0, depth = std::pow(10.0, -10.0 + 7.0 * u.rnd());
        const double off = side * depth * (u.rnd() < 0.1 ? 0.0 : 1.0);
        p = mk(on.x + off * (c.x - on.x), on.y + off * (c.y - on.y), on.z + off * (c.z - on.z));
    }
    const double radius = kRad + (it % 7 == 0 ? (2 * u.rnd() - 1) * 0.9e-4 : 0.0);  // the shell the table vouches for: 1e-4 either side
    return scale(normalized(p), radius);
}

}  // namespace

}  // namespace msm

// Testing hook, host only: the guarantee of the direction table (build_ray_table), checked point by point against the reference's own search.
// For each of `nsamples` points on the radius shell -- random directions, and points placed within 1e-10 .. 1e-3 (relative to the edge) of
// random edges and vertices, on either side -- every candidate of the point's cell that a kernel may accept (the float test, or the FP64
// re-test of a nearly accepted candidate, plus ray_vouches: the very functions the kernels call, search_device.hpp) must be THE answer of
// Octree::get_closest_triangle's first pass (R/octree.cpp:156-178): listed in the leaf the point descends to, and the only listed triangle
// that passes the -1e-8 inside test.  The first candidate of a certified sub-cell (internal.hpp: kRayWBits) is taken as the kernels take it, without
// a test, and counts in [1]; what ray_find returns for the point is held to the same standard.  report: [0] points, [1] accepted by the float test, [2] accepted only by the FP64 re-test, [3] left to
// the complete search, [4] VIOLATIONS (must be 0), [5] triangles the table cannot use, [6] triangles with exclusion boxes, [7] simple surface,
// [8] exclusion boxes checked one by one (a point at the centre of the leaf a box stands for must be refused for that triangle, a violation otherwise),
// [9] sampled points whose triangle passed the edge-plane test and was refused by ray_vouches alone.
extern "C" int msm_ray_table_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[10]) {
    using namespace msm;
    TableUnderTest u;
    MSM_TRY(u.build("msm_ray_table_check", xyz, tri, V, T, nsamples, seed, report, 10));
    const FlatOctree &o = u.o;
    const DevTree &dt = u.dt;
    report[7] = o.rays.simple ? 1 : 0;
    if (o.rays.G <= 0) return MSM_OK;
    std::vector<int> guarded;  // triangles with exclusion boxes: every fifth point is placed above one of them
    for (int t = 0; t < T; ++t) {
        if (o.rays.edge[3 * (size_t)t].w >= 2.f) ++report[5];
        else if (__builtin_bit_cast(int32_t, o.rays.edge[3 * (size_t)t + 1].w) >= 0) guarded.push_back(t);
    }
    report[6] = (int64_t)guarded.size();
    // the records themselves: every leaf that meets the shell region of a guarded triangle without listing it must be refused
    for (int t : guarded) {
        const V3 v[3] = {u.vert(t, 0), u.vert(t, 1), u.vert(t, 2)};
        double lo[3], hi[3];
        std::vector<int> lack;
        if (ray_shell_box(v, lo, hi)) lacking_leaves(o, 0, lo, hi, t, 1 << 20, lack);  // (the box build_ray_table looked through)
        for (int leaf : lack) {
            const double4 b = o.nodebox[leaf];
            const V3 centre = mk(b.x + 0.5 * b.w, b.y + 0.5 * b.w, b.z + 0.5 * b.w);
            ++report[8];
            if (ray_vouches(dt, o.rays.edge[3 * (size_t)t + 1], centre)) ++report[4];
        }
    }
    for (int it = 0; it < nsamples; ++it) {
        const V3 p = table_check_point(u, guarded, it);
        ++report[0];
        const std::vector<int> &hits = u.first_pass(p);
        // what a kernel may accept
        float fx, fy, fz;
        bool cert;
        const int4 cell = ray_cell_of(dt, p, fx, fy, fz, cert);
        const std::array<int, 7> cand = u.candidates(cell);
        const double pn = norm(p);
        bool by_float = false, by_fp64 = false, bad = false;
        if (cert) {  // a certified sub-cell: the kernels take the first candidate without a test (counted with the float test's)
            by_float = true;
            if (!(hits.size() == 1 && hits[0] == cell.x)) bad = true;
        }
        const int found = ray_find_in(dt, o.rays.edge.data(), 3, p);  // the search of the kernels that take one point at a time, shortcut included
        if (found >= 0 && !(hits.size() == 1 && hits[0] == found)) bad = true;
        for (int k = 0; k < 7 && cell.x >= 0; ++k) {
            const int t = cand[k];
            if (t < 0) break;
            const float4 e0 = o.rays.edge[3 * (size_t)t], e1 = o.rays.edge[3 * (size_t)t + 1], e2 = o.rays.edge[3 * (size_t)t + 2];
            float least;
            const int lvl = ray_accept_level(e0, e1, e2, fx, fy, fz, least);
            bool ok = lvl == 2;
            const bool fp64 = lvl == 1 && ray_accepts_fp64(u.vert(t, 0), u.vert(t, 1), u.vert(t, 2), p, pn, (double)e0.w - kRayFloatAllowance + 1e-12);
            ok = ok || fp64;
            if (ok && !ray_vouches(dt, e1, p)) ++report[9];
            if (!ok || !ray_vouches(dt, e1, p)) continue;
            (lvl == 2 ? by_float : by_fp64) = true;
            if (!(hits.size() == 1 && hits[0] == t)) bad = true;
        }
        if (bad) ++report[4];
        if (by_float) ++report[1];
        else if (by_fp64) ++report[2];
        else ++report[3];
    }
    return MSM_OK;
}

// Testing hook, host only: what the first-candidate hints of the direction cells (internal.hpp: kRayHintK) are worth, and that they leave the
// candidates alone.  `nsamples` random directions on the radius shell; a point's triangle is the one the reference's first pass returns, found as
// msm_ray_table_check finds it (the only listed triangle of the point's leaf that passes the inside test; a point without one counts in [0] only).
// report: [0] points, [1] points whose triangle is ray_cell_of(...).x, [2] points whose triangle is the cell's first stored candidate (hints ignored),
// [3] points whose triangle is anywhere in the cell's list (ray_more included), [4] CELLS WHOSE DECODED CANDIDATES DIFFER FROM THE STORED ONES in some
// sub-cell (must be 0: the same ids, the others in their stored order, a ray_more reference where it was, a first candidate whenever there is one),
// [5] cells, [6] cells that use ray_more, [7] kRayHintK (3).  cells (may be NULL): the cell array as stored, 4 x [5] words, when cells_cap holds it.
extern "C" int msm_ray_hint_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[8], int32_t *cells,
                                  int64_t cells_cap) {
    using namespace msm;
    TableUnderTest u;
    MSM_TRY(u.build("msm_ray_hint_check", xyz, tri, V, T, nsamples, seed, report, 8));
    const FlatOctree &o = u.o;
    const DevTree &dt = u.dt;
    report[7] = kRayHintK;
    if (o.rays.G <= 0) return MSM_OK;
    const size_t ncell = o.rays.cell.size();
    report[5] = (int64_t)ncell;
    MSM_TRY(u.copy_cells(cells, cells_cap));
    for (size_t c = 0; c < ncell; ++c) {
        const int4 raw = o.rays.cell[c], ids = ray_cell_ids(raw);
        if (ids.x >= 0 && ids.w < -1) ++report[6];
        const int stored[4] = {ids.x, ids.y, ids.z, ids.w};
        bool same = true;
        for (int k = 0; k < 4; ++k) same = same && stored[k] < T && (stored[k] >= -1 || (k == 3 && -2 - stored[k] < (int)o.rays.more.size()));
        for (int su = 0; su < kRayHintK && same; ++su)
            for (int sv = 0; sv < kRayHintK && same; ++sv) {
                const int h = ray_cell_hint(raw, su, sv);
                const int4 d = ray_cell_first(raw, h);
                const int got[4] = {d.x, d.y, d.z, d.w};
                same = got[0] == stored[h] && (stored[0] < 0 || got[0] >= 0);
                for (int k = 0, j = 1; k < 4; ++k)  // the others behind it, in their stored order
                    if (k != h) same = same && got[j++] == stored[k];
            }
        if (!same) ++report[4];
    }
    for (int it = 0; it < nsamples; ++it) {
        V3 p;
        const int answer = u.random_point(p);
        ++report[0];
        if (answer < 0) continue;
        float fx, fy, fz;
        size_t at;
        int su, sv;
        if (!ray_cell_at(dt, p, fx, fy, fz, at, su, sv)) continue;
        const int4 first = ray_cell_of(dt, p, fx, fy, fz), ids = ray_cell_ids(o.rays.cell[at]);
        if (first.x == answer) ++report[1];
        if (ids.x == answer) ++report[2];
        const std::array<int, 7> list = u.candidates(ids);
        if (std::find(list.begin(), list.end(), answer) != list.end()) ++report[3];
    }
    return MSM_OK;
}

// Testing hook, host only: how deep in a cell's candidate list the answer sits, in the order a kernel tries the candidates: ray_cell_of(...).x (the hinted
// first candidate), .y, .z, then .w or the four ids of the cell's ray_more entry.  The points and the answer are msm_ray_hint_check's (`nsamples` random
// directions on the radius shell; the one triangle the reference's first pass returns, a point without one counts in [0] only).  What k_unary_rays does
// behind a first-candidate miss is sized by these shares (unary_kernels.hip: round A, round T).
// report: [0] points, [1..5] points whose triangle is at position 0, 1, 2, 3, 4 of that order, [6] at position 5 or beyond, [7] not listed.
extern "C" int msm_ray_depth_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[8]) {
    using namespace msm;
    TableUnderTest u;
    MSM_TRY(u.build("msm_ray_depth_check", xyz, tri, V, T, nsamples, seed, report, 8));
    const FlatOctree &o = u.o;
    const DevTree &dt = u.dt;
    if (o.rays.G <= 0) return MSM_OK;
    for (int it = 0; it < nsamples; ++it) {
        V3 p;
        const int answer = u.random_point(p);
        ++report[0];
        if (answer < 0) continue;
        float fx, fy, fz;
        const int4 c = ray_cell_of(dt, p, fx, fy, fz);
        if (c.x < 0) continue;  // (off the shell: no cell)
        const std::array<int, 7> list = u.candidates(c);
        int at = 7;
        for (int k = 0; k < 7 && list[k] >= 0; ++k)
            if (list[k] == answer) {
                at = k;
                break;
            }
        ++report[at == 7 ? 7 : 1 + std::min(at, 5)];
    }
    return MSM_OK;
}

// Testing hook, host only: the certificates of the direction cells (internal.hpp: kRayWBits; ray_table.cpp has the proof), point by point.  A point in a
// certified sub-cell -- placed by ray_cell_at, as a kernel places it -- is taken by the kernels for its first candidate unseen, so that candidate must pass the FP64
// edge-plane test at the threshold the table's proof asks for (ray_accepts_fp64 at the stored threshold less the float allowance, as the kernels' FP64 re-test
// runs it) and must be THE answer of the reference's first pass (msm_ray_table_check: the only listed triangle of the point's leaf that passes the inside test).
// Points: `nsamples` random directions, then placed ones -- within 1e-6 of a cell of sub-cell borders and of cell borders (one coordinate, and both: the corners),
// of cube-face edges and corners (on either side: beyond |u| = 1 the point belongs to the neighbouring face, and float rounding decides which), through mesh
// vertices, and through edge midpoints displaced by 1e-9 of the way to the third vertex, either way.
// report: [0] points, [1] points in a certified sub-cell, [2] OF THOSE, POINTS WHOSE FIRST CANDIDATE FAILS THE FP64 TEST, [3] OF THOSE, POINTS FOR WHICH THE REFERENCE'S
// FIRST PASS DOES NOT RETURN IT (both must be 0), [4] sub-cells, [5] certified sub-cells, [6] cells, [7] placed points.  cells: as msm_ray_hint_check.
extern "C" int msm_ray_cert_check(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int32_t nsamples, uint64_t seed, int64_t report[8], int32_t *cells,
                                  int64_t cells_cap) {
    using namespace msm;
    TableUnderTest u;
    MSM_TRY(u.build("msm_ray_cert_check", xyz, tri, V, T, nsamples, seed, report, 8));
    const FlatOctree &o = u.o;
    const DevTree &dt = u.dt;
    if (o.rays.G <= 0) return MSM_OK;
    const size_t ncell = o.rays.cell.size();
    report[6] = (int64_t)ncell;
    MSM_TRY(u.copy_cells(cells, cells_cap));
    for (size_t c = 0; c < ncell; ++c)
        for (int su = 0; su < kRayHintK; ++su)
            for (int sv = 0; sv < kRayHintK; ++sv) {
                ++report[4];
                if (ray_cell_cert(o.rays.cell[c], su, sv)) ++report[5];
            }
    auto rnd = [&]() { return u.rnd(); };
    const int G = o.rays.G;
    auto on_face = [&](int f, double uu, double v) {  // the direction of face coordinates (u, v), as ray_cell_at reads them
        const int a = f >> 1;
        double comp[3];
        comp[a] = (f & 1) ? -1.0 : 1.0, comp[(a + 1) % 3] = uu, comp[(a + 2) % 3] = v;
        return mk(comp[0], comp[1], comp[2]);
    };
    auto check = [&](V3 p) {
        p = scale(normalized(p), kRad);
        ++report[0];
        float fx, fy, fz;
        bool cert;
        const int4 first = ray_cell_of(dt, p, fx, fy, fz, cert);
        if (!cert) return;
        ++report[1];
        const int t = first.x;
        if (t < 0 || t >= T) {
            ++report[2], ++report[3];
            return;
        }
        if (!ray_accepts_fp64(u.vert(t, 0), u.vert(t, 1), u.vert(t, 2), p, norm(p), (double)o.rays.edge[3 * (size_t)t].w - kRayFloatAllowance + 1e-12)) ++report[2];
        const std::vector<int> &hits = u.first_pass(p);
        if (!(hits.size() == 1 && hits[0] == t)) ++report[3];
    };
    for (int it = 0; it < nsamples; ++it) check(u.random_direction());
    const int64_t before = report[0];
    const double cellw = 2.0 / G;
    auto nudge = [&]() { return rnd() < 0.2 ? 0.0 : (rnd() < 0.5 ? -1.0 : 1.0) * 1e-6 * rnd() * cellw; };
    auto border = [&](bool cell_border) {  // a coordinate next to a sub-cell border (or a cell border) of a random cell
        const int i = (int)(rnd() * G) % G, s = cell_border ? 0 : 1 + (int)(rnd() * (kRayHintK - 1)) % (kRayHintK - 1);
        return -1 + 2.0 * (i + (double)s / kRayHintK) / G + nudge();
    };
    auto rim = [&]() { return (rnd() < 0.5 ? -1.0 : 1.0) + nudge(); };
    for (int it = 0; it < 6000; ++it) {
        const int f = (int)(rnd() * 6) % 6, kind = it % 6;
        double uu = 2 * rnd() - 1, v = 2 * rnd() - 1;
        if (kind == 0) uu = border(false);                          // a sub-cell border
        else if (kind == 1) uu = border(false), v = border(false);  // a sub-cell corner
        else if (kind == 2) v = border(true);                       // a cell border
        else if (kind == 3) uu = border(true), v = border(it % 12 < 6);  // a cell corner, or a cell border meeting a sub-cell border
        else if (kind == 4) (rnd() < 0.5 ? uu : v) = rim();         // a cube-face edge
        else uu = rim(), v = rim();                                 // a cube-face corner
        check(on_face(f, uu, v));
    }
    for (int j = 0; j < std::min((int)V, 3000); ++j) check(vtx(xyz, V, V <= 3000 ? j : (int)(rnd() * V) % V));
    for (int it = 0; it < 3000; ++it) {
        const int t = (int)(rnd() * T) % T, k = (int)(rnd() * 3) % 3;
        const V3 a = u.vert(t, k), b = u.vert(t, (k + 1) % 3), c = u.vert(t, (k + 2) % 3);
        const V3 mid = mk(0.5 * (a.x + b.x), 0.5 * (a.y + b.y), 0.5 * (a.z + b.z));
        const double off = (it & 1) ? 1e-9 : -1e-9;
        check(mk(mid.x + off * (c.x - mid.x), mid.y + off * (c.y - mid.y), mid.z + off * (c.z - mid.z)));
    }
    report[7] = report[0] - before;
    return MSM_OK;
}

// [host] testing hook: a signature of the whole direction table of a mesh (build_octree + build_ray_table, no GPU) -- every word the kernels are given.
// out: [0] G (0: no table, and every count is zero), [1] simple surface, [2] built with certificates, [3..6] elements of cell, edge, more, excl, [7] [8] the
// bit patterns of r2lo and r2hi, [9..12] 64-bit FNV-1a (the constants of msm_octree_signature) over the raw bytes of cell, edge, more, excl.
extern "C" int msm_ray_table_signature(const double *xyz, const int32_t *tri, int32_t V, int32_t T, uint64_t out[13]) {
    using namespace msm;
    TableUnderTest u;
    MSM_TRY(u.build("msm_ray_table_signature", xyz, tri, V, T, 0, 0, reinterpret_cast<int64_t *>(out), 13));
    const RayTable &r = u.o.rays;
    auto fnv = [](const void *p, size_t bytes) {
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < bytes; ++i) {
            h ^= static_cast<const unsigned char *>(p)[i];
            h *= 1099511628211ull;
        }
        return h;
    };
    out[0] = (uint64_t)r.G, out[1] = r.simple ? 1 : 0, out[2] = r.certs ? 1 : 0;
    out[3] = r.cell.size(), out[4] = r.edge.size(), out[5] = r.more.size(), out[6] = r.excl.size();
    out[7] = __builtin_bit_cast(uint64_t, r.r2lo), out[8] = __builtin_bit_cast(uint64_t, r.r2hi);
    out[9] = fnv(r.cell.data(), r.cell.size() * sizeof(int4)), out[10] = fnv(r.edge.data(), r.edge.size() * sizeof(float4));
    out[11] = fnv(r.more.data(), r.more.size() * sizeof(int4)), out[12] = fnv(r.excl.data(), r.excl.size() * sizeof(int4));
    return MSM_OK;
}
