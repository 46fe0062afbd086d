// smooth_plan_client.cpp -- msmhip::ResamplePlan::smoothing of include/msmhip.hpp as a compiled program (g++ + libmsmhip.so, no Python in the loop), for
// comparison with newmsm_amd.ResamplePlan.smoothing on the same inputs (tests/test_cpp_smooth_plan.py).
//
//   smooth_plan_client <in.bin> <out.bin>      file format: host_mirror.cpp.  in: xyz, tri (AoS; one sphere is orig and sphLow), data (D x V), excl (V),
//   sigma (1).  out: sizes, row_ptr / col / val / div of the masked plan, out64, out32 (the float32 result widened: the container holds doubles), mask,
//   plain (the plan without a mask applied to data).
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
        const double sigma = F["sigma"].at(0);
        Matrix out64, plain;
        std::vector<double> mask, div;
        std::vector<float> out32;
        SparseWeights w;
        std::vector<int32_t> sizes;
        {
            Mesh sphere(ctx, F["xyz"], I["tri"]);
            ResamplePlan plan = ResamplePlan::smoothing(sphere, sphere, sigma, &F["excl"]);
            sizes = {plan.nvertices_in(), plan.nvertices_out(), (int32_t)plan.nnz(), plan.longest_row()};
            w = plan.weights();
            div = plan.divisors();
            out64 = plan.apply(data, &mask);
            out32 = plan.apply(std::vector<float>(data.begin(), data.end()));
            if (!plan.masked()) throw std::runtime_error("the plan forgot its mask");
            plain = ResamplePlan::smoothing(sphere, sphere, sigma).apply(data);
            bool refused = false;
            try {
                ResamplePlan::smoothing(sphere, sphere, 0.0);
            } catch (const Error &e) {
                refused = e.code == MSM_ERR_INVALID && std::string(e.what()).find("sigma") != std::string::npos;
            }
            if (!refused) throw std::runtime_error("sigma = 0 was not refused");
            refused = false;
            try {
                plan.apply_labels(std::vector<int32_t>((size_t)plan.nvertices_in(), 1));
            } catch (const Error &e) {
                refused = e.code == MSM_ERR_INVALID;
            }
            if (!refused) throw std::runtime_error("labels through a smoothing plan were not refused");
        }
        put(out, "sizes", "i4", sizes);
        put(out, "row_ptr", "i4", w.row_ptr);
        put(out, "col", "i4", w.col);
        put(out, "val", "f8", w.val);
        put(out, "div", "f8", div);
        put(out, "out64", "f8", out64);
        put(out, "out32", "f8", std::vector<double>(out32.begin(), out32.end()));
        put(out, "mask", "f8", mask);
        put(out, "plain", "f8", plain);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "smooth_plan_client: %s\n", e.what());
        return 1;
    }
    return 0;
}
