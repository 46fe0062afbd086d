// dedrift_client.cpp -- dedrift_group of include/msmhip_dedrift.hpp as a compiled program (g++ + libmsmhip.so, no Python in the loop), for
// comparison with newmsm_amd/dedrift.py on the same inputs (tests/test_cpp_dedrift.py).
//
//   dedrift_client <in.bin> <out.bin>      file format: host_mirror.cpp.  in: template_xyz, template_tri, sizes {S, D, subject to write}, and per
//   subject s orig<s>, reg<s>, tri<s>, data<s>.  out: W, drift, the chosen subject's corrected / resampled / distortion, mean, stdev, cc, dice,
//   figures {cc_mean[D], dice_mean[D], areal mean, max, 95, 98, shape mean, max}.
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "msmhip_dedrift.hpp"

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
        const int S = I["sizes"][0], pick = I["sizes"][2];
        std::vector<DedriftSubject> subjects(S);
        for (int s = 0; s < S; ++s) {
            const std::string k = std::to_string(s);
            subjects[s].orig = F["orig" + k];
            subjects[s].reg = F["reg" + k];
            subjects[s].tri = I["tri" + k];
            subjects[s].data = F["data" + k];
        }
        Context ctx(0);
        const DedriftResult r = dedrift_group(ctx, F["template_xyz"], I["template_tri"], subjects, F["percentile"][0]);
        std::ofstream out(argv[2], std::ios::binary);
        put(out, "W", "f8", r.W);
        put(out, "drift", "f8", r.drift);
        put(out, "corrected", "f8", r.corrected[pick]);
        put(out, "resampled", "f8", r.resampled[pick]);
        put(out, "distortion", "f8", r.distortion[pick]);
        put(out, "mean", "f8", r.mean);
        put(out, "stdev", "f8", r.stdev);
        put(out, "cc", "f8", r.cc);
        put(out, "dice", "f8", r.dice);
        std::vector<double> fig(r.cc_mean);
        fig.insert(fig.end(), r.dice_mean.begin(), r.dice_mean.end());
        for (double v : {r.areal_mean, r.areal_max, r.areal_95, r.areal_98, r.shape_mean, r.shape_max}) fig.push_back(v);
        put(out, "figures", "f8", fig);
        std::puts("ok");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "dedrift_client failed: %s\n", e.what());
        return 1;
    }
}
