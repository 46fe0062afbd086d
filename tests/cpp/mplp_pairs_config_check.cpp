// mplp_pairs_config_check.cpp -- the opt-in of MPLP over the pair tables in include/msmhip_config.hpp's levels_from_config, as a compiled program (built
// by tests/test_mplp_pairs_cpu.py; no GPU): with mplp and mplp_pairs a --regoption=1 / --dopt=MPLP level is the pairwise model with
// LevelOptions::mplp_pairs; without mplp_pairs the FastPD-only message comes; the other optimisers are what they were.  argv[1]: a configuration with
// %DOPT% and %REG% in the places of the optimiser and the regulariser mode.  Prints "ok".
#include <cstdio>
#include <fstream>
#include <sstream>

#include "msmhip_config.hpp"

using namespace msmhip;

static std::string with(std::string text, const std::string &dopt, const std::string &reg) {
    text.replace(text.find("%DOPT%"), 6, dopt);
    text.replace(text.find("%REG%"), 5, reg);
    return text;
}

static int fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

// the message levels_from_config ends with ("" when it returns), and the first level's options
static std::string outcome(const std::string &text, bool mplp, bool pairs, LevelOptions *o) {
    try {
        const std::vector<LevelSpec> levels = levels_from_config(parse_config(text), 1, nullptr, nullptr, false, false, nullptr, mplp, pairs);
        if (levels.empty()) return "no levels";
        *o = levels[0].options;
        return "";
    } catch (const ConfigError &e) {
        return e.what();
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return fail("usage: mplp_pairs_config_check <configuration>");
    std::ifstream in(argv[1]);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    LevelOptions o;
    if (!outcome(with(text, "MPLP", "1"), true, true, &o).empty()) return fail("--dopt=MPLP --regoption=1 refused with both switches");
    if (!o.pairwise || !o.mplp_pairs || o.mplp || o.fusion || o.mciters != 5 || o.cost.regularisermode != 1) return fail("the level's options with both switches");
    if (outcome(with(text, "MPLP", "1"), true, false, &o).find("--regoption=1") == std::string::npos) return fail("without mplp_pairs the FastPD-only message stays");
    if (outcome(with(text, "MPLP", "1"), false, true, &o) != "Unrecognized optimiser") return fail("mplp_pairs without mplp takes --dopt=MPLP");
    if (outcome(with(text, "MPLP", "1"), false, false, &o) != "Unrecognized optimiser") return fail("--dopt=MPLP taken without a switch");
    for (int sw = 0; sw < 4; ++sw) {  // the other optimisers, and MPLP over triplets, are what they were under every combination of the switches
        const bool mplp = sw & 1, pairs = sw & 2;
        if (!outcome(with(text, "HOCR", "3"), mplp, pairs, &o).empty() || !o.fusion || o.pairwise || o.mplp || o.mplp_pairs) return fail("HOCR");
        if (!outcome(with(text, "MCMC", "3"), mplp, pairs, &o).empty() || o.fusion || o.pairwise || o.mplp || o.mplp_pairs) return fail("MCMC");
        if (!outcome(with(text, "FastPD", "1"), mplp, pairs, &o).empty() || o.fusion || !o.pairwise || o.mplp || o.mplp_pairs) return fail("FastPD");
        if (outcome(with(text, "HOCR", "1"), mplp, pairs, &o).find("--regoption=1") == std::string::npos) return fail("HOCR with --regoption=1");
        if (outcome(with(text, "ELC", "3"), mplp, pairs, &o) != "Unrecognized optimiser") return fail("an unknown optimiser");
        const std::string triplets = outcome(with(text, "MPLP", "3"), mplp, pairs, &o);
        if (mplp ? (!triplets.empty() || !o.mplp || o.pairwise || o.mplp_pairs) : triplets != "Unrecognized optimiser") return fail("MPLP over triplets");
    }
    std::printf("ok\n");
    return 0;
}
