// octree.cpp -- host construction of the triangle search structure.
//
// newresampler::Octree (R/octree.cpp:31-141, R/node.cpp) grows a pointer tree by inserting triangles
// one at a time: a leaf that reaches MAX_TRIANGLES entries is split when the split heuristic holds,
// and its triangles are handed down to every child whose closed box overlaps their AABB.  Which leaf
// a query lands in -- and so which triangles are candidates -- depends on that insertion history, so
// the same incremental procedure is run here, on index-based nodes, and then laid out as flat arrays
// for the GPU:
//   node[]      int4 per node (first child, or leaf entry range + mask block + depth) -> descent is arithmetic + 1 load/level
//   leaf_tri[]  triangle ids of all leaves, contiguous per leaf, in insertion (= ascending id) order, padded to x8
//   cone[]      float4 per (padded) leaf entry: conservative bounding cone of the triangle (cheap reject test; filled on the
//               GPU together with recs[], kernels.hip k_build_recs / k_expand_cones)
//   mask[]      per leaf 64 x 64-bit: which entries a query inside each of the leaf's 4x4x4 sub-cells can hit
//               (filled on the GPU, kernels.hip k_build_masks)
//   recs[]      128-byte record per triangle for the exact test
// The direction ("ray") table that simple surfaces get on top of the tree is built in ray_table.cpp.
#include <algorithm>
#include <cstdlib>
#include <deque>

#include "host_parallel.hpp"
#include "internal.hpp"

namespace msm {

namespace {

struct BNode {
    int first_child = -1;  // index of child (0,0,0); children are consecutive in (i,j,k) order
    int parent = -1;
    double b[3][3];  // per axis: lower, middle, upper (Node::bounds, R/node.h:42)
    std::vector<int32_t> tris;
    // running sums of the split heuristic over `tris` (the reference recomputes them over the whole leaf at every
    // insertion past MAX_TRIANGLES, R/octree.cpp:71-93; the node's midpoints never change, so they can be kept)
    int total_size = 0, num_split = 0;
};

struct Builder {
    const double *xyz;
    const int32_t *tri;
    int V, T;
    std::deque<BNode> nodes;
    std::vector<double> box;  // per triangle: lo[3], hi[3]
    const double *bxp = nullptr;  // = box.data(), or another builder's boxes (worker threads share them)

    void precompute_boxes() {
        box.resize((size_t)6 * T);
        bxp = box.data();
        parallel_chunks(T, T < 20000 ? 1 : std::min(host_workers(), 8), [&](int, int t0, int t1) {
            for (int t = t0; t < t1; ++t) {
                double *lo = &box[(size_t)6 * t], *hi = lo + 3;
                for (int a = 0; a < 3; ++a) lo[a] = hi[a] = xyz[a * V + tri[t]];
                for (int k = 1; k < 3; ++k)
                    for (int a = 0; a < 3; ++a) {
                        double c = xyz[a * V + tri[k * T + t]];
                        if (c < lo[a]) lo[a] = c;
                        if (c > hi[a]) hi[a] = c;
                    }
            }
        });
    }
    void aabb(int t, double lo[3], double hi[3]) const {
        const double *b = &bxp[(size_t)6 * t];
        for (int a = 0; a < 3; ++a) {
            lo[a] = b[a];
            hi[a] = b[3 + a];
        }
    }
    // Node::can_contain, R/node.cpp:108-116
    bool overlaps(int n, const double lo[3], const double hi[3]) const {
        const BNode &nd = nodes[n];
        for (int a = 0; a < 3; ++a)
            if (hi[a] < nd.b[a][0] || lo[a] > nd.b[a][2]) return false;
        return true;
    }
    // Node::make_children, R/node.cpp:84-106
    void split(int n) {
        int base = (int)nodes.size();
        for (int c = 0; c < 8; ++c) {
            BNode ch;
            const int oct[3] = {(c >> 2) & 1, (c >> 1) & 1, c & 1};
            for (int a = 0; a < 3; ++a) {
                ch.b[a][0] = nodes[n].b[a][oct[a]];
                ch.b[a][2] = nodes[n].b[a][oct[a] + 1];
                ch.b[a][1] = (ch.b[a][0] + ch.b[a][2]) / 2.0;
            }
            ch.parent = n;
            ch.tris.reserve(kMaxTriangles);
            nodes.push_back(std::move(ch));
        }
        nodes[n].first_child = base;
    }
    // Octree::add_triangle, R/octree.cpp:65-141
    void add(int n, int t, const double lo[3], const double hi[3]) {
        if (nodes[n].first_child < 0) {
            nodes[n].tris.push_back(t);
            {
                int split_size = 8;
                for (int d = 0; d < 3; ++d)  // containing_oct: coordinate < middle, R/node.cpp:70-82
                    if ((lo[d] < nodes[n].b[d][1]) == (hi[d] < nodes[n].b[d][1])) split_size >>= 1;
                nodes[n].total_size += split_size;
                if (split_size != 8) ++nodes[n].num_split;
            }
            const int num = (int)nodes[n].tris.size();
            if (num < kMaxTriangles) return;
            if (!(nodes[n].num_split > 0 && nodes[n].total_size < 3 * num)) return;
            split(n);
            std::vector<int32_t> held;
            held.swap(nodes[n].tris);  // clear_triangles() after redistribution
            for (int tt : held) {
                double tlo[3], thi[3];
                aabb(tt, tlo, thi);
                for (int c = 0; c < 8; ++c)
                    if (overlaps(nodes[n].first_child + c, tlo, thi)) add(nodes[n].first_child + c, tt, tlo, thi);
            }
        } else {
            for (int c = 0; c < 8; ++c)
                if (overlaps(nodes[n].first_child + c, lo, hi)) add(nodes[n].first_child + c, t, lo, hi);
        }
    }

    // ---- the same tree, top down ------------------------------------------------------------------------------
    // Inserting the triangles one by one is equivalent to this: a node sees, in ascending id, every triangle whose box
    // overlaps it (when a leaf splits, the triangles it holds are handed down in order and all later ones follow in
    // order; a child never sees anything else, nor in another order).  It stays a leaf unless the split heuristic
    // holds at some insertion from the MAX_TRIANGLES-th on -- the first such insertion splits it, and from then on only
    // its children matter.  So a node is decided by one scan of its list, and its children by the sub-lists of the
    // WHOLE list that overlap them: no per-triangle descent, and independent subtrees can be built on separate threads.
    // `nodes` must hold node n with its box; children are appended to `nodes`.
    void build_down(int n, std::vector<int32_t> &list) {
        int total_size = 0, num_split = 0;
        bool splits = false;
        const int len = (int)list.size();
        for (int i = 0; i < len; ++i) {
            const double *bx = &bxp[(size_t)6 * list[i]];
            int split_size = 8;
            for (int d = 0; d < 3; ++d)
                if ((bx[d] < nodes[n].b[d][1]) == (bx[3 + d] < nodes[n].b[d][1])) split_size >>= 1;
            total_size += split_size;
            if (split_size != 8) ++num_split;
            if (i + 1 >= kMaxTriangles && num_split > 0 && total_size < 3 * (i + 1)) {
                splits = true;
                break;
            }
        }
        if (!splits) {
            nodes[n].tris = std::move(list);
            return;
        }
        split(n);
        const int first = nodes[n].first_child;
        std::vector<int32_t> sub[8];
        distribute(n, list, sub);
        std::vector<int32_t>().swap(list);  // the parent's list is not needed below
        for (int c = 0; c < 8; ++c) build_down(first + c, sub[c]);
    }

    // The children's lists of a node that has just been split: child c receives, in order, every triangle of `list` whose box
    // overlaps the child's box (Node::can_contain on the child).  The eight tests of a triangle share their comparisons: per
    // axis the child box is the parent's [lower, middle] or [middle, upper], so twelve comparisons decide all eight.
    void distribute(int n, const std::vector<int32_t> &list, std::vector<int32_t> sub[8]) const {
        const BNode &nd = nodes[n];
        const size_t guess = list.size() / 5 + 8;
        for (int c = 0; c < 8; ++c) sub[c].reserve(guess);
        for (const int32_t t : list) {
            const double *bx = &bxp[(size_t)6 * t];
            unsigned half[3];  // bit 0: overlaps the lower half along the axis, bit 1: the upper half
            for (int a = 0; a < 3; ++a)
                half[a] = (!(bx[3 + a] < nd.b[a][0] || bx[a] > nd.b[a][1]) ? 1u : 0u) | (!(bx[3 + a] < nd.b[a][1] || bx[a] > nd.b[a][2]) ? 2u : 0u);
            for (int c = 0; c < 8; ++c)
                if ((half[0] >> ((c >> 2) & 1) & 1u) && (half[1] >> ((c >> 1) & 1) & 1u) && (half[2] >> (c & 1) & 1u)) sub[c].push_back(t);
        }
    }
};

// build_down over the whole mesh; the subtrees below the first two levels are built on worker threads, each in its own
// node store, and spliced into b.nodes afterwards (only the order of the nodes differs from the serial build).
void build_top_down(Builder &b) {
    auto tick_ = std::chrono::steady_clock::now();
    std::vector<int32_t> all(b.T);
    for (int t = 0; t < b.T; ++t) all[t] = t;
    const int workers = host_workers();
    if (workers == 1 || b.T < 20000) {  // threads cost more than they save on small meshes
        b.build_down(0, all);
        return;
    }
    struct Job {
        int node;
        std::vector<int32_t> list;
    };
    // levels 0 and 1: decide and split here, collect the (node, list) pairs of the next level instead of recursing
    std::vector<Job> frontier, next;
    frontier.push_back(Job{0, std::move(all)});
    for (int level = 0; level < 2; ++level) {
        next.clear();
        // decide every node of the level (a scan that stops at the split), create the children of those that split ...
        std::vector<std::pair<int, int>> todo;  // (job, slot in next) of the children to fill
        for (size_t jn = 0; jn < frontier.size(); ++jn) {
            Job &j = frontier[jn];
            int total_size = 0, num_split = 0;
            bool splits = false;
            const int len = (int)j.list.size();
            for (int i = 0; i < len && !splits; ++i) {
                const double *bx = &b.bxp[(size_t)6 * j.list[i]];
                int split_size = 8;
                for (int d = 0; d < 3; ++d)
                    if ((bx[d] < b.nodes[j.node].b[d][1]) == (bx[3 + d] < b.nodes[j.node].b[d][1])) split_size >>= 1;
                total_size += split_size;
                if (split_size != 8) ++num_split;
                splits = i + 1 >= kMaxTriangles && num_split > 0 && total_size < 3 * (i + 1);
            }
            if (!splits) {
                b.nodes[j.node].tris = std::move(j.list);
                continue;
            }
            b.split(j.node);
            const int first = b.nodes[j.node].first_child;
            for (int c = 0; c < 8; ++c) {
                todo.push_back({(int)jn, (int)next.size()});
                next.push_back(Job{first + c, {}});
            }
        }
        // ... and fill the children's lists (one pass over the parent's list per split node) on the worker threads
        parallel_for((int)todo.size() / 8, workers, [&](int k) {
            const Job &j = frontier[todo[8 * k].first];
            std::vector<int32_t> sub[8];
            b.distribute(j.node, j.list, sub);
            for (int c = 0; c < 8; ++c) next[todo[8 * k + c].second].list = std::move(sub[c]);
        });
        frontier.swap(next);
    }
    TICK("octree: top levels");
    // every remaining job builds its subtree in a private node store whose node 0 stands for the job's node
    std::vector<Builder> part;
    part.reserve(frontier.size());
    for (const Job &j : frontier) {
        part.push_back(Builder{b.xyz, b.tri, b.V, b.T, {}, {}, b.bxp});
        part.back().nodes.push_back(b.nodes[j.node]);
    }
    parallel_for((int)frontier.size(), workers, [&](int k) { part[k].build_down(0, frontier[k].list); });
    TICK("octree: subtrees");
    for (size_t k = 0; k < part.size(); ++k) {
        const int root = frontier[k].node, base = (int)b.nodes.size() - 1;  // local i > 0 -> base + i
        auto global = [&](int i) { return i == 0 ? root : base + i; };
        std::deque<BNode> &ln = part[k].nodes;
        b.nodes[root].tris = std::move(ln[0].tris);
        b.nodes[root].first_child = ln[0].first_child < 0 ? -1 : global(ln[0].first_child);
        for (size_t i = 1; i < ln.size(); ++i) {
            BNode nd = std::move(ln[i]);
            nd.parent = global(nd.parent);
            if (nd.first_child >= 0) nd.first_child = global(nd.first_child);
            b.nodes.push_back(std::move(nd));
        }
    }
}

}  // namespace

void build_octree(const double *xyz, const int32_t *tri, int V, int T, FlatOctree &out) {
    auto tick_ = std::chrono::steady_clock::now();
    Builder b{xyz, tri, V, T, {}, {}, nullptr};
    b.precompute_boxes();
    TICK("octree: boxes");
    BNode root;
    for (int a = 0; a < 3; ++a) {
        root.b[a][0] = -kBounds;
        root.b[a][2] = kBounds;
        root.b[a][1] = (root.b[a][0] + root.b[a][2]) / 2.0;
    }
    root.tris.reserve(kMaxTriangles);
    b.nodes.push_back(std::move(root));
    const char *incremental = std::getenv("MSMHIP_INCREMENTAL_OCTREE");  // the literal restatement, kept for cross-checks
    if (incremental && incremental[0] == '1') {
        for (int t = 0; t < T; ++t) {  // initialize_tree, R/octree.cpp:42-63
            double lo[3], hi[3];
            b.aabb(t, lo, hi);
            b.add(0, t, lo, hi);
        }
    } else {
        build_top_down(b);
    }

    TICK("octree: insertion");
    out.rays.simple = false;  // decided together with the ray table (build_ray_table), which only the cost kernels need
    out.rays.G = 0;
    out.rays.cell.clear();
    out.rays.edge.clear();

    // Leaf entries are padded to multiples of 8 (id -1, a cone nothing passes): 8 cones = one 128-byte line.
    const int n = (int)b.nodes.size();
    out.node.resize(n);
    out.nodebox.resize(n);
    out.parent.resize(n);
    out.leaf_tri.clear();
    out.nmask_blocks = 0;
    int64_t leaves = 0, maxleaf = 0, refs = 0;
    std::vector<int> depth(n, 0);
    int maxdepth = 0;
    for (int i = 0; i < n; ++i) {
        const BNode &nd = b.nodes[i];
        out.parent[i] = nd.parent;
        if (i > 0) depth[i] = depth[nd.parent] + 1;  // children always follow their parent in the node array
        maxdepth = std::max(maxdepth, depth[i]);
        out.nodebox[i] = make_double4(nd.b[0][0], nd.b[1][0], nd.b[2][0], nd.b[0][2] - nd.b[0][0]);
        if (nd.first_child >= 0) {
            out.node[i] = make_int4(nd.first_child, 0, -1, depth[i]);
        } else {
            const int cnt = (int)nd.tris.size();
            const int mblock = (cnt >= 1 && cnt <= 64) ? out.nmask_blocks++ : -1;
            out.node[i] = make_int4(-cnt - 1, (int)out.leaf_tri.size(), mblock, depth[i]);
            for (int e = 0; e < ((cnt + 7) & ~7); ++e) {
                out.leaf_tri.push_back(e < cnt ? nd.tris[e] : -1);
            }
            ++leaves;
            refs += cnt;
            maxleaf = std::max<int64_t>(maxleaf, (int64_t)cnt);
        }
    }
    // dense top grid: every node at depth <= grid_depth that is a leaf, or sits at grid_depth, owns a cube of cells
    out.grid_depth = std::min(maxdepth, 6);
    const int G = 1 << out.grid_depth;
    out.grid.assign((size_t)G * G * G, 0);
    {
        struct Item { int node, depth, ix, iy, iz; };
        std::vector<Item> stack{{0, 0, 0, 0, 0}};
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            const BNode &nd = b.nodes[it.node];
            if (nd.first_child < 0 || it.depth == out.grid_depth) {
                const int span = 1 << (out.grid_depth - it.depth);
                for (int x = 0; x < span; ++x)
                    for (int y = 0; y < span; ++y)
                        for (int z = 0; z < span; ++z)
                            out.grid[((size_t)(it.ix * span + x) * G + (it.iy * span + y)) * G + (it.iz * span + z)] = it.node;
            } else {
                for (int c = 0; c < 8; ++c)
                    stack.push_back({nd.first_child + c, it.depth + 1, 2 * it.ix + ((c >> 2) & 1), 2 * it.iy + ((c >> 1) & 1), 2 * it.iz + (c & 1)});
            }
        }
    }
    TICK("octree: flatten + grid");
    out.stats[0] = n;
    out.stats[1] = leaves;
    out.stats[2] = maxdepth;
    out.stats[3] = refs;
    out.stats[4] = maxleaf;
}

}  // namespace msm

// [host] testing hook: the search tree of a mesh without a GPU -- its statistics and a signature of its leaves (box and
// triangle list of every leaf, independent of the order in which the nodes were created)
extern "C" int msm_octree_signature(const double *xyz, const int32_t *tri, int32_t V, int32_t T, int64_t stats[5], uint64_t *signature) {
    if (!xyz || !tri || V <= 0 || T <= 0) return msm::fail(MSM_ERR_INVALID, "msm_octree_signature: bad arguments");
    msm::FlatOctree o;
    msm::build_octree(xyz, tri, V, T, o);
    if (stats) std::copy(o.stats, o.stats + 5, stats);
    if (signature) {
        uint64_t sum = 0;
        for (size_t n = 0; n < o.node.size(); ++n) {
            if (o.node[n].x >= 0) continue;
            uint64_t h = 1469598103934665603ull;
            auto mix = [&](uint64_t v) {
                for (int k = 0; k < 8; ++k) {
                    h ^= (v >> (8 * k)) & 0xff;
                    h *= 1099511628211ull;
                }
            };
            const double4 b = o.nodebox[n];
            for (double d : {b.x, b.y, b.z, b.w}) mix((uint64_t)__builtin_bit_cast(uint64_t, d));
            for (int e = 0; e < -o.node[n].x - 1; ++e) mix((uint64_t)o.leaf_tri[o.node[n].y + e]);
            sum += h;
        }
        *signature = sum;
    }
    return MSM_OK;
}
