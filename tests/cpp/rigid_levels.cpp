// rigid_levels.cpp -- include/msmhip_config.hpp's levels_from_config(..., rigid = true) as a compiled program: rigid_levels <config file | NONE> <D>
// prints every level (RIGID ones with what Rigid_cost_function reads) and the skipped ones as one JSON line (tests/test_rigid_cpu.py).  Host logic only.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "msmhip_config.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::stringstream ss;
    ss << in.rdbuf();
    const msmhip::Config c = msmhip::parse_config(ss.str(), std::string(argv[1]) == "NONE");
    std::vector<std::pair<int, std::string>> skipped;
    const auto levels = msmhip::levels_from_config(c, std::atoi(argv[2]), nullptr, &skipped, false, true);
    std::printf("{\"skipped\": %zu, \"levels\": [", skipped.size());
    for (size_t i = 0; i < levels.size(); ++i) {
        const msmhip::LevelSpec &l = levels[i];
        std::printf("%s{\"method\": \"%s\", \"data_order\": %d, \"sigma_in\": %.17g, \"sigma_ref\": %.17g, \"iters\": %d, \"simmeasure\": %d, \"stepsize\": %.17g, "
                    "\"gradsampling\": %.17g}",
                    i ? ", " : "", l.rigid ? "RIGID" : "DISCRETE", l.data_order, l.sigma_in, l.sigma_ref, l.options.iters, l.options.cost.simmeasure, l.stepsize,
                    l.gradsampling);
    }
    std::printf("]}\n");
    return 0;
}
