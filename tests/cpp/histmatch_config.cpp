// histmatch_config.cpp -- include/msmhip_config.hpp as a compiled program for --IN / --INc: histmatch_config <config file> <D> <optin 0|1> [groupwise]
// prints what levels_from_config / group_levels_from_config hand to the level loops (IntensityNorm, Exclusion, the number of levels) or the error, as
// one JSON line, for comparison with newmsm_amd/config.py (tests/test_histmatch_cpu.py).  Host logic only.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "msmhip_group_registration.hpp"

int main(int argc, char **argv) {
    if (argc != 4 && argc != 5) return 2;
    std::ifstream in(argv[1]);
    std::stringstream ss;
    ss << in.rdbuf();
    const bool optin = std::atoi(argv[3]) != 0;
    try {
        const msmhip::Config c = msmhip::parse_config(ss.str(), false);
        msmhip::IntensityNorm n;
        bool varnorm = false;
        const size_t levels = argc == 5 ? msmhip::group_levels_from_config(c, &varnorm, optin ? &n : nullptr).size()
                                        : msmhip::levels_from_config(c, std::atoi(argv[2]), &varnorm, nullptr, false, false, optin ? &n : nullptr).size();
        const msmhip::Exclusion e = msmhip::exclusion_from_config(c);
        std::printf("{\"levels\": %zu, \"varnorm\": %s, \"intensity\": %s, \"cut\": %s, \"excl\": %s}\n", levels, varnorm ? "true" : "false", n.on ? "true" : "false",
                    n.cut ? "true" : "false", e.on ? "true" : "false");
        return 0;
    } catch (const msmhip::ConfigError &e) {
        std::string m = e.what();
        for (char &ch : m)
            if (ch == '"') ch = '\'';
        std::printf("{\"error\": \"%s\"}\n", m.c_str());
        return 0;
    }
}
