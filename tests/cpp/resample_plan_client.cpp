// resample_plan_client.cpp -- msmhip::ResamplePlan of include/msmhip.hpp as a compiled program (g++ + libmsmhip.so, no Python in the loop), for
// comparison with newmsm_amd.ResamplePlan on the same inputs (tests/test_cpp_resample_plan.py).
//
//   resample_plan_client <in.bin> <out.bin>      file format: host_mirror.cpp.  in: in_xyz, in_tri, new_xyz, new_tri (AoS), data (D x V_in), excl (V_in),
//   keys (Dk x V_in).  out: row_ptr / col / val of the adaptive plan, out64, out32 (the float32 result widened: the container holds doubles), labels,
//   masked / mask of the plan with excl, nearest, bary (the barycentric plan applied to in_xyz's three coordinate rows), sizes.
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "msmhip.hpp"

using namespace msmhip;

static std::map<std::string, std::vector<double>> F;
static std::map<std::string, std::vector<int32_t>> I;

static void read_bag(const char *path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error(std::string("cannot open ") + path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream hs(line);
        std::string name, dtype;
        size_t n;
        hs >> name >> dtype >> n;
        if (dtype == "f8") {
            F[name].resize(n);
            in.read(reinterpret_cast<char *>(F[name].data()), (std::streamsize)(n * 8));
        } else {
            I[name].resize(n);
            in.read(reinterpret_cast<char *>(I[name].data()), (std::streamsize)(n * 4));
        }
    }
}
template <class T>
static void put(std::ofstream &out, const std::string &name, const char *dtype, const std::vector<T> &v) {
    out << name << " " << dtype << " " << v.size() << "\n";
    out.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    try {
        read_bag(argv[1]);
        Context ctx(0);
        std::ofstream out(argv[2], std::ios::binary);
        const Matrix &data = F["data"];
        Matrix out64, nearest, bary, masked;
        std::vector<double> mask;
        std::vector<float> out32;
        std::vector<int32_t> labels;
        SparseWeights w;
        std::vector<int32_t> sizes;
        {
            Mesh in_mesh(ctx, F["in_xyz"], I["in_tri"]), new_mesh(ctx, F["new_xyz"], I["new_tri"]);
            ResamplePlan plan(in_mesh, new_mesh);
            sizes = {plan.nvertices_in(), plan.nvertices_out(), (int32_t)plan.nnz(), plan.longest_row()};
            w = plan.weights();
            out64 = plan.apply(data);
            out32 = plan.apply(std::vector<float>(data.begin(), data.end()));
            labels = plan.apply_labels(I["keys"], -1);
            ResamplePlan with_mask(in_mesh, new_mesh, MSM_RESAMPLE_ADAP_BARY, &F["excl"]);
            masked = with_mask.apply(data, &mask);
            ResamplePlan nn(in_mesh, new_mesh, MSM_RESAMPLE_NEAREST);
            nearest = nn.apply(data);
            ResamplePlan bc(in_mesh, new_mesh, MSM_RESAMPLE_BARYCENTRIC);
            bary = bc.apply(to_soa(F["in_xyz"]));
            bool refused = false;
            try {
                ResamplePlan bad(in_mesh, new_mesh, 7);
            } catch (const Error &e) {
                refused = e.code == MSM_ERR_INVALID && std::string(e.what()).find("method") != std::string::npos;
            }
            if (!refused) throw std::runtime_error("an unknown method was not refused");
        }
        put(out, "sizes", "i4", sizes);
        put(out, "row_ptr", "i4", w.row_ptr);
        put(out, "col", "i4", w.col);
        put(out, "val", "f8", w.val);
        put(out, "out64", "f8", out64);
        put(out, "out32", "f8", std::vector<double>(out32.begin(), out32.end()));
        put(out, "labels", "i4", labels);
        put(out, "masked", "f8", masked);
        put(out, "mask", "f8", mask);
        put(out, "nearest", "f8", nearest);
        put(out, "bary", "f8", bary);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "resample_plan_client: %s\n", e.what());
        return 1;
    }
    return 0;
}
