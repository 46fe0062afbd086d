// excl_config.cpp -- include/msmhip_config.hpp as a compiled program for --excl / --cutthr: excl_config <config file> <D> [groupwise] prints what
// exclusion_from_config hands to the level loops, with the number of levels (or the error), as one JSON line, for comparison with
// newmsm_amd/config.py (tests/test_trans_excl_cpu.py).  Host logic only.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "msmhip_group_registration.hpp"

int main(int argc, char **argv) {
    if (argc != 3 && argc != 4) return 2;
    std::ifstream in(argv[1]);
    std::stringstream ss;
    ss << in.rdbuf();
    try {
        const msmhip::Config c = msmhip::parse_config(ss.str(), false);
        const size_t levels = argc == 4 ? msmhip::group_levels_from_config(c).size() : msmhip::levels_from_config(c, std::atoi(argv[2])).size();
        const msmhip::Exclusion e = msmhip::exclusion_from_config(c);
        std::printf("{\"levels\": %zu, \"excl\": %s, \"cutthr\": [%.17g, %.17g], \"message\": \"%s\"}\n", levels, e.on ? "true" : "false", e.lower, e.upper,
                    msmhip::excl_with_weightings_message());
        return 0;
    } catch (const msmhip::ConfigError &e) {
        std::string m = e.what();
        for (char &ch : m)
            if (ch == '"') ch = '\'';
        std::printf("{\"error\": \"%s\"}\n", m.c_str());
        return 0;
    }
}
