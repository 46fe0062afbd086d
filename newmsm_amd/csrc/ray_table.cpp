// ray_table.cpp -- host construction of the direction ("ray") table of a simple surface, over the tree octree.cpp builds.
//
// build_ray_table at the end of the file is the list of passes; each pass is a function above it, and the block comment before the first says what
// the table promises.  The table has the same words whatever the number of worker threads (tests/test_ray_table_signature_cpu.py pins them).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "host_parallel.hpp"
#include "ray_table.hpp"
#include "search_device.hpp"  // the cells' decoding (ray_cell_ids, ray_cell_hint, ray_cell_first), which also compiles for the host

namespace msm {

namespace {

// True when every ray from the origin meets exactly one triangle: the mesh is a closed, consistently oriented
// 2-manifold, every face is strictly front- (or every face strictly back-) facing seen from the origin, and the faces'
// solid angles add up to one full sphere (degree of the radial projection = 1).
bool simple_star_surface(const double *xyz, const int32_t *tri, int V, int T) {
    if (T < 4) return false;
    // faces: orientation seen from the origin and solid angle, on worker threads (chunk sums added in chunk order)
    const int workers = T < 20000 ? 1 : host_workers();
    std::vector<double> part_solid(4 * (size_t)std::max(workers, 1), 0.0);
    std::vector<int> part_sign(part_solid.size(), 0);  // +1 / -1: all faces of the chunk face that way; 2: the mesh fails
    parallel_chunks(T, workers, [&](int c, int t0, int t1) {
        double solid = 0.0;
        int sign = 0;
        for (int t = t0; t < t1; ++t) {
            const int id[3] = {tri[t], tri[T + t], tri[2 * T + t]};
            bool bad = id[0] == id[1] || id[1] == id[2] || id[0] == id[2];
            for (int k = 0; k < 3; ++k) bad = bad || id[k] < 0 || id[k] >= V;
            if (bad) {
                sign = 2;
                break;
            }
            const V3 a = vtx(xyz, V, id[0]), b = vtx(xyz, V, id[1]), cc = vtx(xyz, V, id[2]);
            const double la = norm(a), lb = norm(b), lc = norm(cc);
            const double triple = dot(a, cross(b, cc));
            if (!(la > 0 && lb > 0 && lc > 0) || !std::isfinite(triple)) {
                sign = 2;
                break;
            }
            const int s = triple > 1e-12 * la * lb * lc ? 1 : (triple < -1e-12 * la * lb * lc ? -1 : 0);
            if (s == 0 || (sign != 0 && s != sign)) {  // a face seen edge-on or from behind
                sign = 2;
                break;
            }
            sign = s;
            // Van Oosterom-Strackee solid angle of the face
            const double den = la * lb * lc + dot(a, b) * lc + dot(a, cc) * lb + dot(b, cc) * la;
            solid += 2.0 * std::atan2(std::fabs(triple), den);
        }
        part_solid[c] = solid;
        part_sign[c] = sign;
    });
    double solid = 0.0;
    int sign = 0;
    for (size_t c = 0; c < part_solid.size(); ++c) {
        if (part_sign[c] == 0) continue;
        if (part_sign[c] == 2 || (sign != 0 && part_sign[c] != sign)) return false;
        sign = part_sign[c];
        solid += part_solid[c];
    }
    // directed edges u -> v bucketed by u: each must be unique (consistent orientation, manifold) and have its opposite
    // (closed surface).  Buckets hold a vertex's valence (six on an icosphere), so the checks are short scans.
    std::vector<int32_t> ptr((size_t)V + 1, 0);
    for (int k = 0; k < 3; ++k)
        for (int t = 0; t < T; ++t) ++ptr[(size_t)tri[(size_t)k * T + t] + 1];
    for (int v = 0; v < V; ++v) ptr[v + 1] += ptr[v];
    std::vector<int32_t> head((size_t)3 * T), fill(ptr.begin(), ptr.end() - 1);
    for (int t = 0; t < T; ++t)
        for (int k = 0; k < 3; ++k) head[fill[tri[(size_t)k * T + t]]++] = tri[(size_t)((k + 1) % 3) * T + t];
    std::atomic<bool> ok{true};
    parallel_chunks(V, workers, [&](int, int v0, int v1) {
        for (int u = v0; u < v1 && ok.load(std::memory_order_relaxed); ++u)
            for (int e = ptr[u]; e < ptr[u + 1]; ++e) {
                const int v = head[e];
                for (int f = ptr[u]; f < e; ++f)
                    if (head[f] == v) ok.store(false, std::memory_order_relaxed);  // the same directed edge twice
                bool opposite = false;
                for (int f = ptr[v]; f < ptr[v + 1]; ++f) opposite = opposite || head[f] == u;
                if (!opposite) ok.store(false, std::memory_order_relaxed);
            }
    });
    if (!ok.load()) return false;
    const long E = (long)3 * T / 2;
    if ((long)V - E + (long)T != 2) return false;  // sphere topology (all vertices referenced is implied when this holds for a closed manifold)
    return std::fabs(solid - 4.0 * M_PI) < 1e-6;
}

// Per triangle: the in-plane distance from every edge of the triangle beyond which no OTHER triangle of a simple
// surface can pass the reference's inside test.  A same_side product equals 2*area*|edge|*(in-plane distance to that
// edge), so a triangle accepts points up to band = 1e-8 / (2*area*shortest edge) outside its edges; the margin is
// max(1e-5 * longest edge, 1000 * the widest band among all triangles sharing a vertex with this one).
std::vector<double> safe_margins(const double *xyz, const int32_t *tri, int V, int T) {
    std::vector<double> band(T), lmax(T), vband(V, 0.0), margin(T);
    for (int t = 0; t < T; ++t) {
        const int id[3] = {tri[t], tri[T + t], tri[2 * T + t]};
        const V3 a = vtx(xyz, V, id[0]), b = vtx(xyz, V, id[1]), c = vtx(xyz, V, id[2]);
        const double la = norm(sub(b, c)), lb = norm(sub(a, c)), lc = norm(sub(a, b));
        const double area = 0.5 * norm(cross(sub(b, a), sub(c, a)));
        lmax[t] = std::fmax(la, std::fmax(lb, lc));
        const double lmin = std::fmin(la, std::fmin(lb, lc));
        band[t] = (area > 0 && lmin > 0) ? 1e-8 / (2 * area * lmin) : HUGE_VAL;
        if (!(band[t] == band[t])) band[t] = HUGE_VAL;
        for (int k = 0; k < 3; ++k) vband[id[k]] = std::fmax(vband[id[k]], band[t]);
    }
    for (int t = 0; t < T; ++t) {
        const double widest = std::fmax(vband[tri[t]], std::fmax(vband[tri[T + t]], vband[tri[2 * T + t]]));
        const double dist = std::fmax(1e-5 * lmax[t], 1e3 * widest);
        margin[t] = (std::isfinite(dist) && dist < 0.05 * lmax[t]) ? dist : HUGE_VAL;
    }
    return margin;
}

}  // namespace

bool lacking_leaves(const FlatOctree &o, int n, const double lo[3], const double hi[3], int t, int cap, std::vector<int> &lack) {
    const double4 box = o.nodebox[n];
    const double blo[3] = {box.x, box.y, box.z};
    for (int a = 0; a < 3; ++a)
        if (hi[a] < blo[a] || lo[a] > blo[a] + box.w) return true;
    const int4 nd = o.node[n];
    if (nd.x < 0) {
        const int32_t *first = o.leaf_tri.data() + nd.y, *last = first + (-nd.x - 1);
        if (std::find(first, last, t) != last) return true;
        if ((int)lack.size() >= cap) return false;
        lack.push_back(n);
        return true;
    }
    for (int c = 0; c < 8; ++c)
        if (!lacking_leaves(o, nd.x + c, lo, hi, t, cap, lack)) return false;
    return true;
}

bool ray_shell_box(const V3 v[3], double lo[3], double hi[3]) {
    V3 u[3];
    double cosmax = 1.0;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const double n = norm(v[k]);
        ok = ok && n > 0;
        u[k] = scale(v[k], 1.0 / n);
    }
    if (!ok) return false;
    for (int k = 0; k < 3; ++k) cosmax = std::fmin(cosmax, dot(u[k], u[(k + 1) % 3]));
    if (!(cosmax > 0.5)) return false;
    const double rlo = kRad - kRayShell, rhi = kRad + kRayShell;
    const double sag = rhi * (1 - std::sqrt(cosmax)) * (1 + 1e-9) + 1e-9;
    for (int a = 0; a < 3; ++a) lo[a] = HUGE_VAL, hi[a] = -HUGE_VAL;
    for (int k = 0; k < 3; ++k) {
        const double c[3] = {u[k].x, u[k].y, u[k].z};
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::fmin(lo[a], std::fmin(rlo * c[a], rhi * c[a]));
            hi[a] = std::fmax(hi[a], std::fmax(rlo * c[a], rhi * c[a]));
        }
    }
    for (int a = 0; a < 3; ++a) lo[a] -= sag, hi[a] += sag;
    return true;
}

bool ray_certs_enabled() {
    const char *e = std::getenv("MSMHIP_RAY_CERTS");
    return !(e && std::strcmp(e, "off") == 0);
}

bool ray_table_disabled() {
    const char *e = std::getenv("MSMHIP_DISABLE_RAYTABLE");
    return e && e[0] == '1';
}

RayTableMode ray_table_mode() {
    const char *e = std::getenv("MSMHIP_RAYTABLE");
    if (e && std::strcmp(e, "off") == 0) return RayTableMode::off;
    return (e && std::strcmp(e, "sync") == 0) ? RayTableMode::sync : RayTableMode::background;
}

namespace {

// ------------------------------------------------------------------------------------------------
// Ray table (simple surfaces).  On such a surface exactly one triangle t meets the ray through a query p, and
// Octree::get_closest_triangle (R/octree.cpp:156-214) returns t provided that
//   (1) t is listed in the leaf p descends to, and
//   (2) no other listed triangle passes the -1e-8 inside test,
// because a single passing triangle wins whatever its dist_to_point.  Both are settled per triangle here:
//   edge planes  the inward unit normals n_k of the planes through the origin and edge k.  The in-plane distance of
//                the projected point from edge k is at least |projection| * (p^ . n_k) >= rho * (p^ . n_k), rho = distance
//                of the triangle's plane from the origin, so  p^ . n_k >= margin / rho  for k = 0,1,2  implies (2);
//                the stored threshold adds kRayFloatAllowance = 3e-6 for the float evaluation (direction 2e-7, normals 6e-8, dot 2e-7);
//                a kernel may settle what lies inside that allowance with FP64 edge planes (search_device.hpp: ray_accepts_fp64);
//   robustness   every point of the shell kRayShell around radius 100 whose direction lies in t's spherical triangle
//                is within `sag` of the flat triangle scaled to that radius; if every leaf meeting the AABB of that
//                region lists t, (1) holds for every such p.  Up to three leaves that do not list t are recorded as
//                exclusion boxes (ray_excl): (1) then holds for every p outside those leaves, and p's leaf at depth d
//                is found arithmetically (child boxes are exact halvings).  More than kRayExclMax = 7 (two records): a threshold
//                nothing passes.  (With three, 72 of the 81 920 triangles of an ico6 sphere were unusable -- the ones whose box ends
//                on a leaf boundary with 2 x 2 leaves beyond it -- and every sample in them went to the complete search.)
// Record layout (three float4 per triangle): {n0, thr} {n1, bits of the ray_excl index or -1} {n2, 0}.
// The cube-map cells only propose candidates, likeliest first: {c0,c1,c2,c3}, or {c0,c1,c2,-2-k} with c3..c6 in
// ray_more[k]; a miss just means the complete search.  The top bits of c0..c2 say which candidate to try first in each
// sub-cell of the cell (internal.hpp: kRayHintK; search_device.hpp: ray_cell_of hands the cell out in that order).
// ------------------------------------------------------------------------------------------------
constexpr int kRayExclMax = 7;

// What the passes share: the mesh, the tree (read only), the table being filled, and which triangles the table can use.
struct RayBuild {
    const double *xyz;
    const int32_t *tri;
    int V, T, workers;
    const FlatOctree &tree;
    RayTable &rays;
    std::vector<char> usable;  // per triangle: it has edge planes (set by the first pass)
    void corners(int t, V3 v[3]) const {
        for (int k = 0; k < 3; ++k) v[k] = vtx(xyz, V, tri[(size_t)k * T + t]);
    }
};

// The normal of the plane through the origin and edge k of a triangle -- the edge opposite vertex k: same_side(p, v_k, v_k+1, v_k+2),
// R/point.cpp:41-44 -- turned towards v_k, not normalised, and its length: n = a x b as ray_accepts_fp64 forms it (search_device.hpp)
V3 inward_edge_normal(const V3 v[3], int k, double &length) {
    V3 n = cross(v[(k + 1) % 3], v[(k + 2) % 3]);
    if (dot(n, v[k]) < 0) n = scale(n, -1.0);
    length = norm(n);
    return n;
}

// (2): the three edge-plane records of a triangle at threshold thr; false: a degenerate edge plane
bool edge_planes(const V3 v[3], double thr, float4 e[3]) {
    for (int k = 0; k < 3; ++k) {
        double nn;
        V3 n = inward_edge_normal(v, k, nn);
        if (!(nn > 0) || !std::isfinite(nn)) return false;
        n = scale(n, 1.0 / nn);
        e[k] = make_float4((float)n.x, (float)n.y, (float)n.z, (float)thr);
        if (!((double)e[k].w >= thr)) e[k].w = std::nextafterf(e[k].w, 1.f);  // round the threshold up
    }
    return true;
}

// leaf boxes as depth << 24 | ix << 16 | iy << 8 | iz (depth <= 8: coordinates fit 8 bits); false: a leaf below depth 8
bool excl_boxes(const FlatOctree &o, const std::vector<int> &lack, int32_t bx[kRayExclMax]) {
    for (int j = 0; j < kRayExclMax; ++j) bx[j] = -1;
    for (size_t j = 0; j < lack.size(); ++j) {
        const double4 nb = o.nodebox[lack[j]];
        const int d = o.node[lack[j]].w;
        if (d > 8) return false;
        const double size = 2 * kBounds / (double)(1 << d);
        const int ix = (int)std::lround((nb.x + kBounds) / size), iy = (int)std::lround((nb.y + kBounds) / size), iz = (int)std::lround((nb.z + kBounds) / size);
        bx[j] = (d << 24) | (ix << 16) | (iy << 8) | iz;
    }
    return true;
}

// Pass 1, per triangle: the edge planes (2) and, where up to kRayExclMax leaves of the shell region do not list the triangle, its exclusion
// record (1).  Sets rays.edge, rays.excl, the radius range, and b.usable.
void edge_planes_and_exclusions(RayBuild &b, const std::vector<double> &margin) {
    const int T = b.T;
    b.rays.edge.assign((size_t)3 * T, make_float4(0.f, 0.f, 0.f, 2.f));
    b.rays.excl.clear();
    b.rays.more.clear();
    b.rays.r2lo = (kRad - kRayShell) * (kRad - kRayShell);
    b.rays.r2hi = (kRad + kRayShell) * (kRad + kRayShell);
    // exclusion records are collected per chunk and numbered afterwards (chunks are contiguous triangle ranges, so the
    // numbering does not depend on the number of threads)
    struct Chunk {
        std::vector<int4> excl;
        std::vector<int> owner;
    };
    std::vector<Chunk> chunk_out(4 * (size_t)b.workers + 1);
    parallel_chunks(T, b.workers, [&](int ci, int t_begin, int t_end) {
        std::vector<int> lack;
        Chunk &mine = chunk_out[ci];
        for (int t = t_begin; t < t_end; ++t) {
            V3 v[3], s3;
            b.corners(t, v);
            double pd;
            plane_of(v[0], v[1], v[2], s3, pd);
            const double rho = std::fabs(pd);  // distance of the triangle's plane from the origin
            if (!(margin[t] < HUGE_VAL) || !(rho > 0)) continue;
            const double thr = margin[t] / rho * (1 + 1e-6) + kRayFloatAllowance;
            if (!(thr < 0.1)) continue;
            // (1): the shell region above the triangle
            double lo[3], hi[3];
            if (!ray_shell_box(v, lo, hi)) continue;
            lack.clear();
            if (!lacking_leaves(b.tree, 0, lo, hi, t, kRayExclMax, lack)) continue;
            float4 e[3];
            if (!edge_planes(v, thr, e)) continue;
            int excl = -1;
            if (!lack.empty()) {
                int32_t bx[kRayExclMax];
                if (!excl_boxes(b.tree, lack, bx)) continue;
                excl = (int)mine.excl.size();  // chunk-local; renumbered below
                mine.excl.push_back(make_int4(bx[0], bx[1], bx[2], (int)lack.size()));
                mine.owner.push_back(t);
                if (lack.size() > 3) {  // boxes 3..6 in the record that follows
                    mine.excl.push_back(make_int4(bx[3], bx[4], bx[5], bx[6]));
                    mine.owner.push_back(-1);
                }
            }
            e[1].w = __builtin_bit_cast(float, (int32_t)excl);
            e[2].w = 0.f;
            for (int k = 0; k < 3; ++k) b.rays.edge[(size_t)3 * t + k] = e[k];
            b.usable[t] = 1;
        }
    });
    for (const Chunk &c : chunk_out) {
        const int base = (int)b.rays.excl.size();
        for (size_t k = 0; k < c.excl.size(); ++k) {
            b.rays.excl.push_back(c.excl[k]);
            if (c.owner[k] >= 0) b.rays.edge[(size_t)3 * c.owner[k] + 1].w = __builtin_bit_cast(float, (int32_t)(base + (int)k));
        }
    }
}

// A triangle's gnomonic image on cube face f = 2*axis + (negative side) -- (u, v) = the two other components over |major
// component| -- and its edge functions, oriented so that the third vertex is on the positive side.
struct FaceTri {
    double pu[3], pv[3], ex[3], ey[3], ox[3], oy[3], sg[3];
    bool project(const V3 v[3], const double ln[3], int f) {  // false: a vertex is not well in front of the face
        const int a = f >> 1, bb = (a + 1) % 3, cc = (a + 2) % 3;
        const double sgn = (f & 1) ? -1.0 : 1.0;
        for (int k = 0; k < 3; ++k) {
            const double c[3] = {v[k].x, v[k].y, v[k].z};
            const double w = sgn * c[a];
            if (!(w > 0.05 * ln[k])) return false;
            pu[k] = c[bb] / w;
            pv[k] = c[cc] / w;
        }
        return true;
    }
    void edges() {
        for (int k = 0; k < 3; ++k) {
            const int p = (k + 1) % 3, q = (k + 2) % 3;
            ex[k] = pu[q] - pu[p], ey[k] = pv[q] - pv[p], ox[k] = pu[p], oy[k] = pv[p];
            sg[k] = (ex[k] * (pv[k] - oy[k]) - ey[k] * (pu[k] - ox[k])) >= 0 ? 1.0 : -1.0;
        }
    }
    double E(int k, double x, double y) const { return sg[k] * (ex[k] * (y - oy[k]) - ey[k] * (x - ox[k])); }
    bool holds(double x, double y) const { return E(0, x, y) >= 0 && E(1, x, y) >= 0 && E(2, x, y) >= 0; }
};

// a usable triangle that overlaps a cell, and how far the cell's centre is from the triangle's centroid on the face (squared: the rank)
struct Cand {
    uint32_t cell;
    float score;
    int32_t tri;
};

// Pass 2: rasterise the usable triangles onto the cube map -- face f = 2*axis + (negative side); (u, v) = the two other components over
// |major component|.  Sets rays.G; returns the candidates per chunk of triangles, in triangle order, and in count[c + 1] how many cell c has.
std::vector<std::vector<Cand>> rasterise(RayBuild &b, std::vector<int32_t> &count) {
    int G = 8;
    while (G < 512 && (double)G * G * 6 < 4.0 * b.T) G *= 2;
    b.rays.G = G;
    std::vector<std::vector<Cand>> found_by(4 * (size_t)b.workers + 1);
    count.assign((size_t)6 * G * G + 1, 0);
    const double m = 1e-5;  // cells are grown by this much (uv units) before the overlap test
    parallel_chunks(b.T, b.workers, [&](int ci, int t_begin, int t_end) {
        std::vector<Cand> &found = found_by[ci];
        found.reserve((size_t)(t_end - t_begin) * 8);
        for (int t = t_begin; t < t_end; ++t) {
            if (!b.usable[t]) continue;
            V3 v[3];
            b.corners(t, v);
            const double ln[3] = {norm(v[0]), norm(v[1]), norm(v[2])};
            for (int f = 0; f < 6; ++f) {
                FaceTri ft;
                if (!ft.project(v, ln, f)) continue;
                const double *pu = ft.pu, *pv = ft.pv;
                const double umin = std::fmin(pu[0], std::fmin(pu[1], pu[2])) - m, umax = std::fmax(pu[0], std::fmax(pu[1], pu[2])) + m;
                const double vmin = std::fmin(pv[0], std::fmin(pv[1], pv[2])) - m, vmax = std::fmax(pv[0], std::fmax(pv[1], pv[2])) + m;
                if (umax < -1 || umin > 1 || vmax < -1 || vmin > 1) continue;
                auto cellof = [&](double x) { return std::max(0, std::min(G - 1, (int)std::floor((x + 1) * 0.5 * G))); };
                const int iu0 = cellof(umin), iu1 = cellof(umax), iv0 = cellof(vmin), iv1 = cellof(vmax);
                const double gu = (pu[0] + pu[1] + pu[2]) / 3, gv = (pv[0] + pv[1] + pv[2]) / 3;
                ft.edges();
                for (int iu = iu0; iu <= iu1; ++iu)
                    for (int iv = iv0; iv <= iv1; ++iv) {
                        const double x0 = -1 + 2.0 * iu / G - m, x1 = -1 + 2.0 * (iu + 1) / G + m;
                        const double y0 = -1 + 2.0 * iv / G - m, y1 = -1 + 2.0 * (iv + 1) / G + m;
                        bool sep = false;  // a triangle edge with the whole (grown) cell strictly outside
                        for (int k = 0; k < 3 && !sep; ++k)
                            sep = ft.E(k, x0, y0) < 0 && ft.E(k, x1, y0) < 0 && ft.E(k, x0, y1) < 0 && ft.E(k, x1, y1) < 0;
                        if (sep) continue;
                        const double cu = 0.5 * (x0 + x1) - gu, cv = 0.5 * (y0 + y1) - gv;
                        const size_t cell = ((size_t)f * G + iu) * G + iv;
                        found.push_back(Cand{(uint32_t)cell, (float)(cu * cu + cv * cv), t});
                    }
            }
        }
    });
    for (const auto &f : found_by)
        for (const Cand &c : f) ++count[c.cell + 1];
    return found_by;
}

// Pass 3: the candidates bucketed by cell (a counting sort; count becomes the cells' offsets into the result)
std::vector<Cand> bucket(const std::vector<std::vector<Cand>> &found_by, std::vector<int32_t> &count) {
    size_t nfound = 0;
    for (const auto &f : found_by) nfound += f.size();
    for (size_t c = 0; c + 1 < count.size(); ++c) count[c + 1] += count[c];
    std::vector<Cand> cand(nfound);
    std::vector<int32_t> fill(count.begin(), count.end() - 1);
    for (const auto &f : found_by)  // chunk order = triangle order: the same buckets as a serial pass
        for (const Cand &c : f) cand[(size_t)fill[c.cell]++] = c;
    return cand;
}

// Pass 4: every cell's candidates ranked, the first three or four into the cell, the next four into ray_more.  false: the references to
// ray_more would leave the fourth word's field (internal.hpp), and the mesh gets no table.
bool rank_and_fill_cells(RayBuild &b, std::vector<Cand> &cand, const std::vector<int32_t> &count) {
    const size_t ncell = count.size() - 1;
    b.rays.cell.assign(ncell, make_int4(-1, -1, -1, -1));
    parallel_chunks((int)ncell, b.workers, [&](int, int c_begin, int c_end) {
        for (int c = c_begin; c < c_end; ++c)
            std::sort(cand.data() + count[c], cand.data() + count[c + 1],
                      [](const Cand &x, const Cand &y) { return x.score < y.score || (x.score == y.score && x.tri < y.tri); });
    });
    for (size_t c = 0; c < ncell; ++c) {
        const Cand *first = cand.data() + count[c], *last = cand.data() + count[c + 1];
        int32_t *slot = &b.rays.cell[c].x;
        const int ncand = (int)(last - first);
        if (ncand <= 4) {
            for (int k = 0; k < ncand; ++k) slot[k] = first[k].tri;
        } else {
            for (int k = 0; k < 3; ++k) slot[k] = first[k].tri;
            slot[3] = -2 - (int)b.rays.more.size();
            int4 more = make_int4(-1, -1, -1, -1);
            int32_t *ms = &more.x;
            for (int k = 0; k < 4 && 3 + k < ncand; ++k) ms[k] = first[3 + k].tri;
            b.rays.more.push_back(more);
        }
    }
    if (b.rays.more.size() <= (size_t)kRayMaxMore) return true;
    b.rays = RayTable();
    b.rays.simple = true;
    return false;
}

// Pass 5: first-candidate hints (internal.hpp: kRayHintK): per sub-cell, the first of the candidates stored in the cell itself whose
// image on the face holds the sub-cell's centre; none: 0, the ranked order.  Cell by cell, from the cell's own content only.
void hints(RayBuild &b) {
    const int G = b.rays.G;
    parallel_chunks((int)b.rays.cell.size(), b.workers, [&](int, int c_begin, int c_end) {
        for (int c = c_begin; c < c_end; ++c) {
            int4 &cell = b.rays.cell[c];
            const int f = c / (G * G), iu = (c / G) % G, iv = c % G;
            const int ids[4] = {cell.x, cell.y, cell.z, cell.w};
            FaceTri ft[4];
            int state[4] = {0, 0, 0, 0};  // 0: not set up yet, 1: usable, -1: not a candidate of this cell
            auto holds = [&](int j, double x, double y) {
                if (state[j] == 0) {
                    const int t = ids[j];
                    state[j] = -1;
                    if (t >= 0) {  // (a negative w: no candidate, or the ray_more reference)
                        V3 v[3];
                        b.corners(t, v);
                        const double ln[3] = {0.0, 0.0, 0.0};  // (the rasteriser found it on this face: it is in front)
                        if (ft[j].project(v, ln, f)) {
                            ft[j].edges();
                            state[j] = 1;
                        }
                    }
                }
                return state[j] > 0 && ft[j].holds(x, y);
            };
            uint32_t bits[3] = {0u, 0u, 0u};
            for (int su = 0; su < kRayHintK && ids[1] >= 0; ++su)  // (a single candidate: nothing to choose)
                for (int sv = 0; sv < kRayHintK; ++sv) {
                    const double x = -1 + 2.0 * (iu + (su + 0.5) / kRayHintK) / G, y = -1 + 2.0 * (iv + (sv + 0.5) / kRayHintK) / G;
                    uint32_t h = 0;
                    for (int j = 0; j < 4; ++j)
                        if (holds(j, x, y)) {
                            h = (uint32_t)j;
                            break;
                        }
                    bits[su] |= h << (kRayIdBits + 2 * sv);
                }
            const uint32_t idmask = (1u << kRayIdBits) - 1u;
            cell.x = (int32_t)(((uint32_t)cell.x & idmask) | bits[0]);
            cell.y = (int32_t)(((uint32_t)cell.y & idmask) | bits[1]);
            cell.z = (int32_t)(((uint32_t)cell.z & idmask) | bits[2]);
        }
    });
}

// the planes of a triangle that can be certified, as ray_accepts_fp64 forms them: n = a x b turned towards the third vertex, and |n|;
// thr < 0: not to be certified (unusable, an exclusion record, a negative threshold)
struct Planes {
    V3 n[3];
    double nn[3], thr;
};

// the planes of every triangle, once (none when no certificates are written)
std::vector<Planes> certificate_planes(const RayBuild &b, bool certs) {
    std::vector<Planes> planes(certs ? (size_t)b.T : 0);
    parallel_chunks(certs ? b.T : 0, b.workers, [&](int, int t_begin, int t_end) {
        for (int t = t_begin; t < t_end; ++t) {
            Planes &q = planes[t];
            const float4 e0 = b.rays.edge[3 * (size_t)t], e1 = b.rays.edge[3 * (size_t)t + 1];
            q.thr = (b.usable[t] && e0.w < 2.f && e0.w >= 0.f && __builtin_bit_cast(int32_t, e1.w) < 0) ? (double)e0.w : -1.0;
            if (q.thr < 0.0) continue;
            V3 v[3];
            b.corners(t, v);
            for (int k = 0; k < 3; ++k) q.n[k] = inward_edge_normal(v, k, q.nn[k]);
        }
    });
    return planes;
}

// Pass 6: certificates (internal.hpp: kRayWBits): one bit per sub-cell in the top nine bits of w, set when the candidate t that the sub-cell's hint
// names -- the one ray_cell_of hands out first; stored in the cell itself, usable, without an exclusion record (e1.w negative), threshold
// tau = e0.w >= 0 -- satisfies n_k . d^ >= tau, k = 0, 1, 2, in FP64 for the direction through each of the four corners of the sub-cell GROWN
// by kRayCertGuard on every side (face units; n_k as ray_accepts_fp64 forms them, and the very expression it evaluates).  Why four corners
// suffice: {d : n . d >= tau |d|} with tau >= 0 is a convex cone (n . d is linear, tau |d| convex), so is the intersection of the three, and
// every direction of the grown sub-cell is a non-negative combination of its four corner rays (the sub-cell is a rectangle in the face's
// plane, the convex hull of its corners).  What a certificate is worth: tau already holds margin / rho (1 + 1e-6) plus the float test's
// allowance of 3e-6, so a certified direction lies at least as far inside the triangle as one the float test accepts (that test guarantees
// tau minus the allowance; the FP64 evaluation here errs by 1e-15), (2) of the table's guarantee holds for it, and (1) holds everywhere in the
// shell because t has no exclusion record.  At most one listed candidate passes the acceptance test, so a kernel that takes t unseen takes
// what its loop over the candidates would have ended with.
// The guard band.  A kernel places a point by ray_cell_at's float arithmetic.  u / w reaches gu through six roundings of 2^-24 (three
// conversions or products per component -- rsqrt's own error scales all components alike and cancels -- the reciprocal, the product),
// 3.6e-7 of |u / w| <= 1; adding 1 rounds by up to 1.2e-7; the product with G / 2 is exact.  So a point's true (u, v) is within 4.8e-7 face
// units of the one that chose its cell and, gu - iu being exact and its product with kRayHintK good to 2^-24, its sub-cell: for any G.  A
// direction that float rounding gives to the neighbouring cube face has |u| <= 1 + 4.8e-7 there and is clamped into a rim sub-cell, whose
// grown rectangle reaches beyond |u| = 1 by the guard (the direction through such a corner is as good as any other).  kRayCertGuard = 4e-6
// is eight times the bound: 1e-3 of a cell at G = 512, 5e-4 at the G = 256 of an ico6 sphere, a fraction of a per cent of the certificates.
// Cell by cell, from the cell's own content only, as the hints: the same words whatever the number of workers.
void certificates(RayBuild &b) {
    const bool certs = ray_certs_enabled();
    b.rays.certs = certs;
    constexpr double kRayCertGuard = 4e-6;
    constexpr int K = kRayHintK;
    const int G = b.rays.G;
    const std::vector<Planes> planes = certificate_planes(b, certs);
    parallel_chunks((int)b.rays.cell.size(), b.workers, [&](int, int c_begin, int c_end) {
        for (int c = c_begin; c < c_end; ++c) {
            int4 &cell = b.rays.cell[c];
            uint32_t bits = 0u;
            if (certs && ray_cell_ids(cell).x >= 0) {
                const int f = c / (G * G), iu = (c / G) % G, iv = c % G;
                const int a = f >> 1, bb = (a + 1) % 3, cc = (a + 2) % 3;
                // directions through the 2K x 2K grown corner positions, and their lengths (the test is homogeneous in d): index 2 s + (upper side)
                double du[2 * K], dvv[2 * K];
                for (int s = 0; s < K; ++s) {
                    du[2 * s] = -1 + 2.0 * (iu + (double)s / K) / G - kRayCertGuard, du[2 * s + 1] = -1 + 2.0 * (iu + (double)(s + 1) / K) / G + kRayCertGuard;
                    dvv[2 * s] = -1 + 2.0 * (iv + (double)s / K) / G - kRayCertGuard, dvv[2 * s + 1] = -1 + 2.0 * (iv + (double)(s + 1) / K) / G + kRayCertGuard;
                }
                V3 dir[2 * K][2 * K];
                double len[2 * K][2 * K];
                uint64_t have = 0;  // (set up when first asked for)
                auto corner = [&](int i, int j) {
                    if (!((have >> (2 * K * i + j)) & 1ull)) {
                        double comp[3];
                        comp[a] = (f & 1) ? -1.0 : 1.0, comp[bb] = du[i], comp[cc] = dvv[j];
                        dir[i][j] = mk(comp[0], comp[1], comp[2]);
                        len[i][j] = norm(dir[i][j]);
                        have |= 1ull << (2 * K * i + j);
                    }
                };
                auto inside = [&](const Planes &q, int i, int j) {
                    corner(i, j);
                    const V3 &d = dir[i][j];
                    bool ok = true;
                    for (int k = 0; k < 3; ++k) ok = ok && dot(q.n[k], d) >= q.thr * q.nn[k] * len[i][j];
                    return ok;
                };
                // one candidate hinted in every sub-cell, and the whole grown cell inside its cone: every grown sub-cell lies in the grown cell
                const int t0 = ray_cell_first(cell, ray_cell_hint(cell, 0, 0)).x;
                bool one = t0 >= 0 && planes[t0].thr >= 0.0;
                for (int su = 0; su < K && one; ++su)
                    for (int sv = 0; sv < K && one; ++sv) one = ray_cell_first(cell, ray_cell_hint(cell, su, sv)).x == t0;
                if (one && inside(planes[t0], 0, 0) && inside(planes[t0], 2 * K - 1, 0) && inside(planes[t0], 0, 2 * K - 1) && inside(planes[t0], 2 * K - 1, 2 * K - 1)) {
                    for (int su = 0; su < K; ++su)
                        for (int sv = 0; sv < K; ++sv) bits |= 1u << (kRayWBits + 3 * su + sv);
                } else {
                    for (int su = 0; su < K; ++su)
                        for (int sv = 0; sv < K; ++sv) {
                            const int t = ray_cell_first(cell, ray_cell_hint(cell, su, sv)).x;
                            if (t < 0) continue;  // (the ray_more reference: the hinted candidate is not in the cell itself)
                            const Planes &q = planes[t];
                            if (q.thr >= 0.0 && inside(q, 2 * su, 2 * sv) && inside(q, 2 * su + 1, 2 * sv) && inside(q, 2 * su, 2 * sv + 1) && inside(q, 2 * su + 1, 2 * sv + 1))
                                bits |= 1u << (kRayWBits + 3 * su + sv);
                        }
                }
            }
            cell.w = (int32_t)(((uint32_t)cell.w & ((1u << kRayWBits) - 1u)) | bits);
        }
    });
}

}  // namespace

void build_ray_table(const double *xyz, const int32_t *tri, int V, int T, FlatOctree &out) {
    auto tick_ = std::chrono::steady_clock::now();
    out.rays.G = 0;
    out.rays.cell.clear();
    out.rays.edge.clear();
    out.rays.simple = simple_star_surface(xyz, tri, V, T);
    if (!out.rays.simple || ray_table_disabled()) return;
    if (T > kRayMaxTris) return;  // ids beyond the id field of the cell's fourth word: no table, the complete search everywhere
    TICK("simple");
    const std::vector<double> margin = safe_margins(xyz, tri, V, T);
    TICK("margins");
    RayBuild b{xyz, tri, V, T, host_workers(), out, out.rays, std::vector<char>(T, 0)};
    edge_planes_and_exclusions(b, margin);
    TICK("edges+robust");
    std::vector<int32_t> count;
    const std::vector<std::vector<Cand>> found_by = rasterise(b, count);
    TICK("raster");
    std::vector<Cand> cand = bucket(found_by, count);
    TICK("bucket");
    if (!rank_and_fill_cells(b, cand, count)) return;
    TICK("cells");
    hints(b);
    TICK("hints");
    certificates(b);
    TICK("certs");
}

}  // namespace msm
