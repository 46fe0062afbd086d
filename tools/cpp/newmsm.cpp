// newmsm.cpp -- the `newmsm` executable over the MI355X path, host side in C++ (north_star: "host code stays C++ and calls HIP through a thin C-ABI ...
// keeping the `newmsm` CLI, config-file format and sphere.reg / warp output layout").  What CLI/newmsm.cpp:6-59 does with Mesh_registration /
// Group_Mesh_registration, assembled from this repository's headers:
//
//   flags            src/msmOptions.h:59-157 (short and long forms, `--key=value` or `--key value`); -h / --help prints them
//   pairwise         set_input / set_reference (load, recentre, true_rescale to RAD: M/mesh_registration.cpp:416-438), set_anatomical as loaded (:434-438),
//                    -t / --trans: set_transformed, the sphere.reg of an earlier run as loaded (:440-443), the first level's starting point (:136-145),
//                    the configuration through the reference's grammar (msmhip_config.hpp = parse_reg_options :459-784), run_multiresolutions
//                    (msmhip_registration.hpp = :30-50), then <out>sphere.reg<surf>, <out>sphere.LR.reg<surf>, <out>transformed_and_reprojected<data>
//                    (:47-49, :352-408, M/mesh_registration.h:170); with both anatomical meshes also <out>anat.reg.surf.gii (project_anatomical_mesh)
//                    and <out>STRAINS.func.gii (calculate_strains, four rows), always GIFTI (:397-407)
//   -g / --groupwise --meshes / --data path lists (read_ascii_list :871-884), --template, --mask; per subject <out>sphere-<i>.reg<surf>,
//                    <out>sphere-<i>.LR.reg<surf>, <out>transformed_and_reprojected-<i><data> (M/group_mesh_registration.cpp:120-133, .h:79-82)
//   -f               GIFTI (.surf.gii / .func.gii), ASCII (.asc / .dpv), ASCII_MAT (.asc / .txt) as set_output_format names them (:827-842)
//
// --excl / --cutthr of the configuration: exclusion masks in every level's feature preparation (msmhip_registration.hpp: level_features) and, pairwise, in the
// final resampling of save_transformed_data (:371-383).
//
// Outside the path and said so instead of silently dropped: AFFINE / RIGID levels (skipped with a note on stderr unless MSMHIP_RIGID=on runs them),
// --IN / --INc, --excl together with both weightings, VTK output; --trans in groupwise mode is ignored with a note on stderr (CLI/newmsm.cpp:13-27 never
// hands it to a groupwise run); the binary solve of --dopt=HOCR / FastPD is a stand-in (iterated conditional modes: FastPD and ELC are licence-restricted and
// FSL-bound), so a run exercises the path exactly as newmsm would but its labelings are not HOCR's.  tools/register_files.py is the same program in Python;
// tests/test_gpu_registration.py compares their files.
//
// Errors: a MeshregException's message on stderr, exit status 1 (CLI/newmsm.cpp:62-68).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "msmhip_config.hpp"
#include "msmhip_group_registration.hpp"
#include "msmhip_io.hpp"

using namespace msmhip;

namespace {

constexpr double RAD = 100.0;
constexpr double kStrainFitRadius = 2.0;  // calculate_strains(2, in_anat, ANAT_TRANS), M/mesh_registration.cpp:405

struct Flag {
    const char *shortname, *longname, *help;
    bool takes_value;
};
// src/msmOptions.h:59-157, in the reference's order
const Flag kFlags[] = {
    {"-h", "--help", "display this message", false},
    {"-v", "--verbose", "switch on diagnostic messages", false},
    {"-p", "--printoptions", "print configuration file options", false},
    {"-d", "--debug", "run debugging or optimising options", false},
    {"-g", "--groupwise", "run newMSM in groupwise mode", false},
    {"-m", "--meshes", "groupwise mode only; list of paths to input meshes. Needs to be a sphere", true},
    {"-s", "--template", "groupwise mode only; templates sphere for resampling. Needs to be a sphere", true},
    {"-l", "--data", "groupwise mode only; list of paths of the data files", true},
    {"-k", "--mask", "groupwise mode only; mask file path", true},
    {"-M", "--inmesh", "input mesh (available formats: ASCII, GIFTI). Needs to be a sphere", true},
    {"-R", "--refmesh", "reference mesh (available formats: ASCII, GIFTI). Needs to be a sphere. If not included algorithm assumes reference mesh is equivalent input", true},
    {"-a", "--inanat", "input anatomical mesh (must either supply both input and reference anatomical surfaces or none)", true},
    {"-A", "--refanat", "reference anatomical mesh (with both: <out>anat.reg.surf.gii and <out>STRAINS.func.gii are written too)", true},
    {"-i", "--indata", "scalar or multivariate data for input - can be ASCII (.asc,.dpv,.txt) or GIFTI (.func.gii or .shape.gii)", true},
    {"-I", "--refdata", "scalar or multivariate data for reference", true},
    {"-t", "--trans", "Transformed source mesh (output of a previous registration, i.e. sphere.reg.gii): the starting point of the first level", true},
    {"-w", "--inweight", "cost function weighting for input", true},
    {"-W", "--refweight", "cost function weighting for reference", true},
    {"-o", "--out", "output basename", true},
    {"-f", "--format", "format of output files, can be: GIFTI, ASCII or ASCII_MAT", true},
    {"-c", "--conf", "configuration file", true},
    {nullptr, "--device", "the GPU to run on (default 0)", true},
};

void usage() {
    std::cout << "\nnewmsm [options]   (msm-mi355x: newMSM's DISCRETE path on an MI355X)\n\n";
    for (const Flag &f : kFlags) std::cout << "\t" << (f.shortname ? std::string(f.shortname) + "," : std::string()) << f.longname << "\t" << f.help << "\n";
    std::cout << std::endl;
}

struct Options {
    std::map<std::string, std::string> value;  // by long name without the dashes
    bool has(const std::string &k) const { return value.count(k) != 0; }
    std::string get(const std::string &k) const {
        auto it = value.find(k);
        return it == value.end() ? std::string() : it->second;
    }
};

Options parse_command_line(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i], val;
        bool inline_value = false;
        const size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) {
            val = arg.substr(eq + 1);
            arg = arg.substr(0, eq);
            inline_value = true;
        }
        const Flag *hit = nullptr;
        for (const Flag &f : kFlags)
            if (arg == f.longname || (f.shortname && arg == f.shortname)) hit = &f;
        if (!hit) throw Error(MSM_ERR_INVALID, "Option " + arg + " is not an option");  // X_OptionError
        const std::string key = std::string(hit->longname).substr(2);
        if (!hit->takes_value) {
            o.value[key] = "1";
            continue;
        }
        if (!inline_value) {
            if (i + 1 >= argc) throw Error(MSM_ERR_INVALID, "Option " + arg + " requires an argument");
            val = argv[++i];
        }
        o.value[key] = val;
    }
    return o;
}

// recentre + true_rescale (R/mesh.cpp:1198-1255), as Mesh_registration::set_input / set_reference apply them: the mean of the vertices to the origin
// (summed vertex by vertex), every vertex to the radius
Points on_sphere(Points xyz, double rad = RAD) {
    const size_t V = xyz.size() / 3;
    double c[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < V; ++i)
        for (int a = 0; a < 3; ++a) c[a] += xyz[3 * i + a];
    for (int a = 0; a < 3; ++a) c[a] /= (double)V;
    for (size_t i = 0; i < V; ++i) {
        double p[3];
        for (int a = 0; a < 3; ++a) p[a] = xyz[3 * i + a] - c[a];
        const double n = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]), k = rad / n;
        for (int a = 0; a < 3; ++a) xyz[3 * i + a] = p[a] * k;
    }
    return xyz;
}

std::string slurp(const std::string &path) {
    if (path.empty()) return std::string();
    std::ifstream in(path);
    if (!in) throw Error(MSM_ERR_INVALID, "cannot open " + path);
    std::stringstream ss;
    ss << in.rdbuf();
    return ss.str();
}

// Mesh_registration::read_ascii_list, M/mesh_registration.cpp:871-884: the whitespace-separated entries of a text file
std::vector<std::string> read_ascii_list(const std::string &path) {
    std::istringstream in(slurp(path));
    std::vector<std::string> out;
    std::string tok;
    while (in >> tok) out.push_back(tok);
    return out;
}

struct Formats {
    std::string surf, data;
};
Formats output_formats(const std::string &fmt) {  // set_output_format, M/mesh_registration.cpp:827-842
    if (fmt == "GIFTI") return {".surf.gii", ".func.gii"};
    if (fmt == "ASCII") return {".asc", ".dpv"};
    if (fmt == "ASCII_MAT") return {".asc", ".txt"};
    throw Error(MSM_ERR_INVALID, "newmsm: VTK output is not written here (GIFTI, ASCII, ASCII_MAT)");
}

void save_data(const std::string &path, const Points &mesh_xyz, const Matrix &data, int D) {
    const size_t n = path.size();
    if (n >= 4 && path.compare(n - 4, 4, ".dpv") == 0) io::save_dpv(path, mesh_xyz, data);
    else if (n >= 4 && path.compare(n - 4, 4, ".txt") == 0) io::save_matrix(path, data, D);
    else io::save_metric(path, data, D);
}

void note_skipped(const std::vector<std::pair<int, std::string>> &skipped) {
    for (const auto &sk : skipped)
        std::cerr << "newmsm: level " << sk.first + 1 << " (--opt=" << sk.second << ") is outside the path (the affine stage stays on the CPU in newmsm): skipped" << std::endl;
}

// MSMHIP_HISTMATCH=on: --IN / --INc run (histogram matching on the GPU) instead of ending the run with an error
bool histmatch_enabled() {
    const char *env = std::getenv("MSMHIP_HISTMATCH");
    return env && std::string(env) == "on";
}

// MSMHIP_FEATURES=gpu: every level's features are prepared through one msm_level_features call; the same files are written
bool features_gpu_enabled() {
    const char *env = std::getenv("MSMHIP_FEATURES");
    return env && std::string(env) == "gpu";
}

// MSMHIP_MCMC_CHAINS=n (1 ... 256): every iteration of a --dopt=MCMC level runs n chains from n seeds and keeps the labelling with the lowest energy
// (DESIGN.md section 5.16); unset or 1: the single run.  Anything else ends the run with a message and exit status 1.
int mcmc_chains_setting() {
    const char *env = std::getenv("MSMHIP_MCMC_CHAINS");
    if (!env) return 1;
    char *end = nullptr;
    const long n = std::strtol(env, &end, 10);
    if (end == env || *end != '\0' || n < 1 || n > 256)
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MCMC_CHAINS=") + env + ": the number of Monte Carlo chains must be a whole number from 1 to 256");
    return (int)n;
}

// MSMHIP_MCMC_DRAW=gpu (with MSMHIP_MCMC=gpu): the GPU sweeps take their proposals from the draw kernel instead of the host's stream (DESIGN.md section
// 5.16, "Proposals on the device"; the same bytes); unset or host: the host's stream.  Anything else, or gpu without MSMHIP_MCMC=gpu, ends the run with a
// message and exit status 1.
bool mcmc_draw_gpu_setting() {
    const char *env = std::getenv("MSMHIP_MCMC_DRAW");
    if (!env || std::string(env) == "host") return false;
    if (std::string(env) != "gpu")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MCMC_DRAW=") + env + ": the proposals are drawn on the host (host, or unset) or on the device (gpu)");
    const char *mcmc_env = std::getenv("MSMHIP_MCMC");
    if (!mcmc_env || std::string(mcmc_env) != "gpu") throw Error(MSM_ERR_INVALID, "MSMHIP_MCMC_DRAW=gpu draws the proposals of the GPU sweeps: it needs MSMHIP_MCMC=gpu");
    return true;
}

// MSMHIP_GROUP_MCMC=on: a --groupwise configuration with --dopt=MCMC runs, block-coordinate descent over the subjects with the Monte Carlo optimiser on
// every block (an extension); unset: it ends with the reference's message (M/group_mesh_registration.cpp:87).  Anything else ends
// the run with a message and exit status 1.
bool group_mcmc_setting() {
    const char *env = std::getenv("MSMHIP_GROUP_MCMC");
    if (!env) return false;
    if (std::string(env) != "on")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_GROUP_MCMC=") + env + ": the groupwise Monte Carlo optimiser is switched on with MSMHIP_GROUP_MCMC=on (unset: off)");
    return true;
}

// MSMHIP_GROUP_MCMC_PASSES=n (1 ... 64): passes over the subjects per iteration of a groupwise --dopt=MCMC level; unset: 1
int group_mcmc_passes_setting() {
    const char *env = std::getenv("MSMHIP_GROUP_MCMC_PASSES");
    if (!env) return 1;
    char *end = nullptr;
    const long n = std::strtol(env, &end, 10);
    if (end == env || *end != '\0' || n < 1 || n > 64)
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_GROUP_MCMC_PASSES=") + env + ": the number of passes over the subjects must be a whole number from 1 to 64");
    return (int)n;
}

// MSMHIP_MCMC_DRAW for a groupwise --dopt=MCMC run, whose blocks always sweep on the device: gpu, host or unset
bool group_mcmc_draw_setting() {
    const char *env = std::getenv("MSMHIP_MCMC_DRAW");
    if (!env || std::string(env) == "host") return false;
    if (std::string(env) != "gpu")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MCMC_DRAW=") + env + ": the proposals are drawn on the host (host, or unset) or on the device (gpu)");
    return true;
}

// MSMHIP_MPLP_FORBID=on (beside MSMHIP_MPLP=on): a --dopt=MPLP level reads the NaN and +infinity entries of its triplet table as forbidden label
// combinations instead of refusing the table ("Forbidden entries")
bool mplp_forbid_setting(bool mplp) {
    const char *env = std::getenv("MSMHIP_MPLP_FORBID");
    if (env && std::string(env) != "on")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MPLP_FORBID=") + env +
                                         ": the forbidden-entry reading of MPLP's triplet table is switched on with MSMHIP_MPLP_FORBID=on (unset: off)");
    if (env && !mplp) throw Error(MSM_ERR_INVALID, "MSMHIP_MPLP_FORBID=on changes how --dopt=MPLP reads its triplet table: it needs MSMHIP_MPLP=on");
    return env != nullptr;
}

// MSMHIP_MPLP_PAIRS=on (beside MSMHIP_MPLP=on): --dopt=MPLP with --regoption=1 runs, as MPLP over the unary and pair tables of the pairwise model with
// both tables on the device, instead of ending the run with the FastPD-only message
bool mplp_pairs_setting(bool mplp) {
    const char *env = std::getenv("MSMHIP_MPLP_PAIRS");
    if (env && std::string(env) != "on")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MPLP_PAIRS=") + env + ": MPLP over the pair tables of --regoption=1 is switched on with MSMHIP_MPLP_PAIRS=on (unset: off)");
    if (env && !mplp) throw Error(MSM_ERR_INVALID, "MSMHIP_MPLP_PAIRS=on lets --dopt=MPLP run a --regoption=1 level: it needs MSMHIP_MPLP=on");
    return env != nullptr;
}

// MSMHIP_MPLP_ROUND=on (beside MSMHIP_MPLP=on): every iteration of a --dopt=MPLP level rounds the final messages to a labelling after its sweeps
// ("Rounding"), with MSMHIP_MPLP_POLISH=n (0 ... 64, default 8) polish passes.  Returns whether it is on and sets *polish.
bool mplp_round_setting(bool mplp, int *polish) {
    const char *env = std::getenv("MSMHIP_MPLP_ROUND"), *passes = std::getenv("MSMHIP_MPLP_POLISH");
    if (env && std::string(env) != "on")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MPLP_ROUND=") + env + ": the rounding of MPLP's messages is switched on with MSMHIP_MPLP_ROUND=on (unset: off)");
    if (env && !mplp) throw Error(MSM_ERR_INVALID, "MSMHIP_MPLP_ROUND=on rounds the messages of --dopt=MPLP: it needs MSMHIP_MPLP=on");
    *polish = 8;
    if (passes) {
        if (!env) throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MPLP_POLISH=") + passes + " sets the polish passes of the rounding: it needs MSMHIP_MPLP_ROUND=on");
        char *end = nullptr;
        const long n = std::strtol(passes, &end, 10);
        if (end == passes || *end != '\0' || n < 0 || n > 64)
            throw Error(MSM_ERR_INVALID, std::string("MSMHIP_MPLP_POLISH=") + passes + ": the number of polish passes must be a whole number from 0 to 64");
        *polish = (int)n;
    }
    return env != nullptr;
}

// MSMHIP_FUSION=mplp: the binary problem of every label step of a --dopt=HOCR level is solved by MPLP on the device (an extension: DESIGN.md section
// 5.21) instead of the stand-in; icm or unset: the stand-in, today's bytes.  MSMHIP_FUSION_SWEEPS=n (1 ... 256, default 10) and
// MSMHIP_FUSION_POLISH=n (0 ... 64, default 8) set its sweeps and polish passes and need MSMHIP_FUSION=mplp.  Returns whether it is on.
bool fusion_mplp_setting(int *sweeps, int *polish) {
    const char *env = std::getenv("MSMHIP_FUSION");
    if (env && std::string(env) != "mplp" && std::string(env) != "icm")
        throw Error(MSM_ERR_INVALID, std::string("MSMHIP_FUSION=") + env + ": the binary solve of a label step is the stand-in (icm, or unset) or MPLP on the device (mplp)");
    const bool on = env && std::string(env) == "mplp";
    *sweeps = 10, *polish = 8;
    const struct {
        const char *name, *what;
        long lo, hi;
        int *value;
    } counts[2] = {{"MSMHIP_FUSION_SWEEPS", "sweeps", 1, 256, sweeps}, {"MSMHIP_FUSION_POLISH", "polish passes", 0, 64, polish}};
    for (const auto &c : counts) {
        const char *text = std::getenv(c.name);
        if (!text) continue;
        if (!on) throw Error(MSM_ERR_INVALID, std::string(c.name) + "=" + text + " sets the " + c.what + " of a label step's MPLP solve: it needs MSMHIP_FUSION=mplp");
        char *end = nullptr;
        const long n = std::strtol(text, &end, 10);
        if (end == text || *end != '\0' || n < c.lo || n > c.hi)
            throw Error(MSM_ERR_INVALID, std::string(c.name) + "=" + text + ": the number of " + c.what + " must be a whole number from " + std::to_string(c.lo) + " to " +
                                             std::to_string(c.hi));
        *c.value = (int)n;
    }
    return on;
}

int run_pairwise(const Options &o, const Formats &fmt, int device) {
    int fusion_sweeps = 10, fusion_polish = 8;
    const bool fusion_mplp = fusion_mplp_setting(&fusion_sweeps, &fusion_polish);
    const int mcmc_chains = mcmc_chains_setting();
    const bool mcmc_draw_gpu = mcmc_draw_gpu_setting();
    for (const char *flag : {"inmesh", "indata", "refdata"})
        if (o.get(flag).empty()) throw Error(MSM_ERR_INVALID, std::string("newmsm: --") + flag + " is required");
    if (o.get("inanat").empty() != o.get("refanat").empty()) throw Error(MSM_ERR_INVALID, "Error: must supply both anatomical meshes or none");  // CLI/newmsm.cpp:41-43
    auto [ixyz0, itri] = io::load_surface(o.get("inmesh"));
    auto [rxyz0, rtri] = io::load_surface(o.get("refmesh").empty() ? o.get("inmesh") : o.get("refmesh"));
    const Points ixyz = on_sphere(ixyz0), rxyz = on_sphere(rxyz0);
    int D = 0, Dr = 0;
    const Matrix idata = io::load_data(o.get("indata"), &D, (long)(ixyz.size() / 3)), rdata = io::load_data(o.get("refdata"), &Dr, (long)(rxyz.size() / 3));
    if (D != Dr) throw Error(MSM_ERR_INVALID, "Mesh_registration: input and reference data have different numbers of feature rows (" + std::to_string(D) + ", " + std::to_string(Dr) + ")");
    const bool anat = !o.get("inanat").empty();
    bool varnorm = false;
    std::vector<std::pair<int, std::string>> skipped;
    const char *rigid_env = std::getenv("MSMHIP_RIGID");  // "on": AFFINE / RIGID levels run (Rigid_cost_function on the GPU) instead of being skipped
    const bool rigid = rigid_env && std::string(rigid_env) == "on";
    const Config cfg = parse_config(slurp(o.get("conf")), o.get("conf").empty());
    IntensityNorm inorm;  // --IN / --INc: taken when MSMHIP_HISTMATCH=on, refused otherwise
    const char *mplp_env = std::getenv("MSMHIP_MPLP");  // "on": --dopt=MPLP (an extension: DESIGN.md section 5.19) runs instead of "Unrecognized optimiser"
    const bool mplp = mplp_env && std::string(mplp_env) == "on";
    int mplp_polish = 8;
    const bool mplp_round = mplp_round_setting(mplp, &mplp_polish);
    const bool mplp_forbid = mplp_forbid_setting(mplp);
    const bool mplp_pairs = mplp_pairs_setting(mplp);
    std::vector<LevelSpec> levels = levels_from_config(cfg, D, &varnorm, &skipped, anat, rigid, histmatch_enabled() ? &inorm : nullptr, mplp, mplp_pairs);
    const char *mcmc_env = std::getenv("MSMHIP_MCMC");  // "gpu": the --dopt=MCMC levels keep both cost tables on the device and run the sweeps there
    const bool mcmc_gpu = mcmc_env && std::string(mcmc_env) == "gpu";
    if (mcmc_gpu)
        for (LevelSpec &lv : levels) lv.options.mcmc_gpu = true;
    if (mcmc_draw_gpu)
        for (LevelSpec &lv : levels) lv.options.mcmc_draw_gpu = true;
    if (features_gpu_enabled())
        for (LevelSpec &lv : levels) lv.options.features_gpu = true;
    for (LevelSpec &lv : levels) lv.options.mcmc_chains = mcmc_chains;
    for (LevelSpec &lv : levels) lv.options.mplp_round = mplp_round, lv.options.mplp_polish = mplp_polish, lv.options.mplp_forbid = mplp_forbid;
    for (LevelSpec &lv : levels) lv.options.fusion_mplp = fusion_mplp, lv.options.fusion_sweeps = fusion_sweeps, lv.options.fusion_polish = fusion_polish;
    const Exclusion excl = exclusion_from_config(cfg);
    note_skipped(skipped);
    if (levels.empty()) throw Error(MSM_ERR_INVALID, "newmsm: the configuration holds no DISCRETE level");
    Points in_anat, ref_anat;
    Triangles in_anat_tri;
    if (anat) {  // set_anatomical: loaded as they are (in_anat keeps its triangles: its normals serve the strain map)
        std::tie(in_anat, in_anat_tri) = io::load_surface(o.get("inanat"));
        ref_anat = io::load_surface(o.get("refanat")).first;
    }
    Matrix in_w, ref_w;
    int in_wr = 0, ref_wr = 0;
    const bool weighted = !o.get("inweight").empty() && !o.get("refweight").empty();
    if (weighted) {
        in_w = io::load_data(o.get("inweight"), &in_wr, (long)(ixyz.size() / 3));
        ref_w = io::load_data(o.get("refweight"), &ref_wr, (long)(rxyz.size() / 3));
    }
    Points trans;
    if (!o.get("trans").empty()) trans = io::load_surface(o.get("trans")).first;  // set_transformed: as loaded, no recentre, no rescale
    Context ctx(device);
    if (o.has("verbose"))
        std::cout << "This is newMSM's DISCRETE path on an MI355X (msm-mi355x).\nStarting multiresolution with " << levels.size() << " levels." << std::endl;
    if (o.has("verbose") && mcmc_gpu) std::cout << "MCMC sweeps on the GPU." << std::endl;
    if (o.has("verbose") && mcmc_draw_gpu) std::cout << "MCMC proposals drawn on the GPU." << std::endl;
    if (o.has("verbose") && mcmc_chains > 1) std::cout << "MCMC with " << mcmc_chains << " chains per iteration." << std::endl;
    if (o.has("verbose") && features_gpu_enabled()) std::cout << "Level features in one call on the GPU." << std::endl;
    if (o.has("verbose") && fusion_mplp) std::cout << "Label steps solved by MPLP on the GPU (" << fusion_sweeps << " sweeps, " << fusion_polish << " polish passes)." << std::endl;
    const MultiresResult res = run_multiresolutions(ctx, ixyz, itri, idata, rxyz, rtri, rdata, D, levels, varnorm, nullptr, anat ? &in_anat : nullptr,
                                                    anat ? &ref_anat : nullptr, weighted ? &in_w : nullptr, in_wr, weighted ? &ref_w : nullptr, ref_wr,
                                                    o.get("trans").empty() ? nullptr : &trans, excl, inorm);
    const std::string out = o.get("out");
    io::save_surface(out + "sphere.reg" + fmt.surf, res.sphere_reg, itri);  // transform
    const Triangles last_tri = make_mesh_from_icosa(levels.back().data_order).second;
    io::save_surface(out + "sphere.LR.reg" + fmt.surf, res.level_reg.back(), last_tri);  // saveSPH_reg
    Mesh moved(ctx, res.sphere_reg, itri), target(ctx, rxyz, rtri);
    // save_transformed_data (:358-383): with --excl a fresh mask from the native input data keeps the cut out of the resampling; with --IN / --INc the
    // native input data is matched to the native reference data first
    if (inorm.on && o.has("verbose")) std::cout << "Intensity normalise." << std::endl;
    save_data(out + "transformed_and_reprojected" + fmt.data, rxyz, transformed_data(ctx, moved, idata, target, rdata, D, excl, inorm), D);
    if (anat) {  // save_transformed_data's aMSM outputs (:397-407), GIFTI whatever -f says
        const Points anat_reg = project_anatomical_mesh(moved, target, ref_anat);
        io::save_surface(out + "anat.reg.surf.gii", anat_reg, itri);
        if (o.has("verbose")) std::cout << "Calculate strains." << std::endl;
        Mesh in_anat_mesh(ctx, in_anat, in_anat_tri);
        io::save_metric(out + "STRAINS.func.gii", calculate_strains(in_anat_mesh, anat_reg, kStrainFitRadius), 4);
    }
    if (o.has("verbose"))
        for (size_t k = 0; k < res.energies.size(); ++k) {
            std::cout << "level " << k + 1 << ": energies per iteration";
            for (double e : res.energies[k]) std::printf(" %.4f", e);
            std::cout << std::endl;
        }
    return 0;
}

int run_groupwise(const Options &o, const Formats &fmt, int device) {
    int fusion_sweeps = 10, fusion_polish = 8;
    if (fusion_mplp_setting(&fusion_sweeps, &fusion_polish))
        throw Error(MSM_ERR_INVALID, "MSMHIP_FUSION=mplp solves label steps of triplets alone: a --groupwise run (pair factors between the subjects) keeps the stand-in; unset it");
    const bool group_mcmc = group_mcmc_setting();
    const int mcmc_chains = group_mcmc ? mcmc_chains_setting() : 1, mcmc_passes = group_mcmc ? group_mcmc_passes_setting() : 1;
    const bool mcmc_draw_gpu = group_mcmc && group_mcmc_draw_setting();
    for (const char *flag : {"meshes", "template", "data"})
        if (o.get(flag).empty()) throw Error(MSM_ERR_INVALID, std::string("newmsm: --groupwise needs --") + flag);
    const std::vector<std::string> mesh_files = read_ascii_list(o.get("meshes")), data_files = read_ascii_list(o.get("data"));
    if (mesh_files.size() != data_files.size())
        throw Error(MSM_ERR_INVALID, "featurespace::Initialize do not have the same number of datasets and surface meshes");  // M/featurespace.cpp:43-44
    if (o.has("trans")) std::cerr << "newmsm: --trans is not used in groupwise mode: ignored" << std::endl;
    const Config cfg = parse_config(slurp(o.get("conf")), o.get("conf").empty());
    bool varnorm = false;
    IntensityNorm inorm;
    // refuses AFFINE / RIGID levels and optimisers other than HOCR (and, with MSMHIP_GROUP_MCMC=on, MCMC)
    std::vector<GroupLevelSpec> levels = group_levels_from_config(cfg, &varnorm, histmatch_enabled() ? &inorm : nullptr, group_mcmc);
    if (levels.empty()) throw Error(MSM_ERR_INVALID, "newmsm: the configuration holds no DISCRETE level");
    if (features_gpu_enabled())
        for (GroupLevelSpec &lv : levels) lv.options.features_gpu = true;
    for (GroupLevelSpec &lv : levels) lv.options.mcmc_chains = mcmc_chains, lv.options.mcmc_passes = mcmc_passes, lv.options.mcmc_draw_gpu = mcmc_draw_gpu;
    std::vector<std::pair<Points, Triangles>> meshes;
    for (size_t k = 0; k < mesh_files.size(); ++k) {
        if (o.has("verbose")) std::cout << "Mesh #" << k << " is " << mesh_files[k] << std::endl;
        auto [xyz, tri] = io::load_surface(mesh_files[k]);
        meshes.emplace_back(on_sphere(xyz), tri);
    }
    if (o.has("verbose")) std::cout << "Template is " << o.get("template") << std::endl;
    auto [txyz0, ttri] = io::load_surface(o.get("template"));
    const Points txyz = on_sphere(txyz0);
    std::vector<Matrix> datas;
    int D = 0;
    for (size_t k = 0; k < data_files.size(); ++k) {
        int Dk = 0;
        datas.push_back(io::load_data(data_files[k], &Dk, (long)(meshes[k].first.size() / 3)));
        if (k == 0) D = Dk;
        else if (Dk != D) throw Error(MSM_ERR_INVALID, "newmsm: the subjects' data have different numbers of feature rows");
    }
    std::vector<double> mask;
    if (!o.get("mask").empty()) {
        int Dm = 0;
        const Matrix m = io::load_data(o.get("mask"), &Dm, (long)(txyz.size() / 3));
        mask.assign(m.begin(), m.begin() + (long)(txyz.size() / 3));  // the first row
    }
    Context ctx(device);
    if (o.has("verbose"))
        std::cout << "This is newMSM's groupwise DISCRETE path on an MI355X (msm-mi355x).\nStarting multiresolution with " << levels.size() << " levels." << std::endl;
    if (o.has("verbose") && features_gpu_enabled()) std::cout << "Level features in one call on the GPU." << std::endl;
    if (o.has("verbose") && cfg.dopt == "MCMC")
        std::cout << "Groupwise MCMC, subject by subject: " << mcmc_chains << " chains per block, " << mcmc_passes << " passes per iteration, proposals drawn on the "
                  << (mcmc_draw_gpu ? "GPU" : "host") << "." << std::endl;
    const GroupMultiresResult res = run_group_multiresolutions(ctx, meshes, datas, D, txyz, ttri, levels, varnorm, mask.empty() ? nullptr : &mask, nullptr,
                                                               exclusion_from_config(cfg), inorm);
    const Triangles last_tri = make_mesh_from_icosa(levels.back().data_order).second;
    Mesh target(ctx, txyz, ttri);
    const std::string out = o.get("out");
    for (size_t s = 0; s < meshes.size(); ++s) {
        const std::string i = std::to_string(s);
        io::save_surface(out + "sphere-" + i + ".reg" + fmt.surf, res.sphere_regs[s], meshes[s].second);            // transform
        io::save_surface(out + "sphere-" + i + ".LR.reg" + fmt.surf, res.level_regs.back()[s], last_tri);           // saveSPH_reg
        Mesh moved(ctx, res.sphere_regs[s], meshes[s].second);
        save_data(out + "transformed_and_reprojected-" + i + fmt.data, txyz, metric_resample(moved, datas[s], target), D);  // save_transformed_data
    }
    if (o.has("verbose"))
        for (size_t k = 0; k < res.energies.size(); ++k) {
            std::cout << "level " << k + 1 << ": energies per iteration";
            for (double e : res.energies[k]) std::printf(" %.4f", e);
            std::cout << std::endl;
        }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        const Options o = parse_command_line(argc, argv);
        if (o.has("help") || argc == 1) {
            usage();
            return 0;
        }
        if (o.has("verbose")) std::cout << "This is newMSM v1.0 on msm-mi355x." << std::endl;
        if (o.has("printoptions")) {
            std::cout << "The configuration grammar is the reference's (Mesh_registration::parse_reg_options, M/mesh_registration.cpp:459-784): one --key=value or --flag per "
                         "line, '#' comments; see include/msmhip_config.hpp for the keys." << std::endl;
            return 0;
        }
        if (o.get("out").empty()) throw Error(MSM_ERR_INVALID, "newmsm: --out is required");
        const Formats fmt = output_formats(o.has("format") ? o.get("format") : std::string("GIFTI"));
        const int device = o.has("device") ? std::atoi(o.get("device").c_str()) : 0;
        return o.has("groupwise") ? run_groupwise(o, fmt, device) : run_pairwise(o, fmt, device);
    } catch (const std::exception &e) {  // MeshregException: the message, exit status 1 (CLI/newmsm.cpp:62-68)
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
