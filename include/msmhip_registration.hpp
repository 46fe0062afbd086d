// msmhip_registration.hpp -- one resolution level of a discrete registration driven through msmhip.hpp, the way newMSM's
// callers drive the path with the Monte Carlo optimiser:
//     Mesh_registration::run_discrete_opt             M/mesh_registration.cpp:164-232
//     NonLinearSRegDiscreteModel::Initialize           M/DiscreteModel.cpp:63-108
//     NonLinearSRegDiscreteModel::setupCostFunction    M/DiscreteModel.cpp:216-262
//     NonLinearSRegDiscreteModel::applyLabeling        M/DiscreteModel.cpp:264-269
//     MCMC::optimise                                   M/mcmc_opt.h:31-134
// Header only, C++17, no HIP headers.  newmsm_amd/registration.py is the same loop in Python (used by the parity tests, which
// also run it over the oracle); tests/test_cpp_host.py checks that the two give identical results.
#ifndef MSMHIP_REGISTRATION_HPP
#define MSMHIP_REGISTRATION_HPP

#include <chrono>
#include <cmath>
#include <iostream>
#include <map>
#include <memory>
#include <string>

#include "msmhip.hpp"

namespace msmhip {

// wall-clock seconds and call counts per phase of the loops below, under the names newmsm_amd/registration.py uses ("get_source_data",
// "unary_table", "fusion_moves", "optimiser", "total_cost", "sphere_project_warp", "unfold", "metric_resample", "smooth_data", ...)
struct PhaseClock {
    std::map<std::string, double> seconds;
    std::map<std::string, long> calls;
    template <class Fn>
    static auto timed(PhaseClock *c, const char *name, Fn &&fn) {
        if (!c) return fn();
        const auto t0 = std::chrono::steady_clock::now();
        struct Stop {
            PhaseClock *c;
            const char *name;
            std::chrono::steady_clock::time_point t0;
            ~Stop() {
                c->seconds[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                ++c->calls[name];
            }
        } stop{c, name, t0};
        return fn();
    }
};

struct LevelOptions {
    int sg_order = -1;  // sampling grid resolution; cp_order + 2 when negative
    int iters = 3;      // --it
    int mciters = 200;  // --mciters
    double mcparam = 0.8;
    uint64_t seed = 0;  // iteration i draws from std::mt19937(seed + i); the reference seeds from std::random_device
    double labeldist = 0.5;
    bool rescale_labels = false;
    Parameters cost;    // kind, similarity measure, regulariser
    // false: MCMC::optimise over the unary and T x L^3 triplet tables.  true: the label loop of Fusion::optimize (I/Fusion/Fusion.h:136-229),
    // per label step ONE msm_cost_triplet_octets for the 8 T combinations -- how --dopt=HOCR drives the path -- with a stand-in for the
    // licence-restricted binary solve (msm_fusion_icm_step, icm_passes passes): the path is exercised as HOCR would, the result is not HOCR's
    bool fusion = false;
    int icm_passes = 5;
    // with fusion (an extension; what MSMHIP_FUSION=mplp, MSMHIP_FUSION_SWEEPS=n and MSMHIP_FUSION_POLISH=n ask of the executables): the
    // binary problem of a label step is solved by MPLP -- fusion_sweeps sweeps from x = 0, then the rounding with fusion_polish polish passes -- in one
    // launch behind the step's own kernel (DiscreteCostFunction::fusion_mplp_step) instead of the stand-in; nothing is queued ahead then
    bool fusion_mplp = false;
    int fusion_sweeps = 10, fusion_polish = 8;
    // true (an extension, not newMSM's; what --dopt=MPLP asks for under MSMHIP_MPLP=on): max-product linear programming over the MCMC optimiser's two
    // tables, mciters sweeps per iteration from the zero labelling (DiscreteCostFunction::mplp_optimise: the tables stay on the device)
    bool mplp = false;
    // with mplp: an iteration rounds the final messages to a labelling after its sweeps -- the conditioned decode and mplp_polish polish passes, then
    // one polish call on the winner (DiscreteCostFunction::mplp_round; what MSMHIP_MPLP_ROUND=on and MSMHIP_MPLP_POLISH=n ask of the executables)
    bool mplp_round = false;
    int mplp_polish = 8;
    // with mplp: NaN and +infinity entries of the triplet table are forbidden label combinations instead of a refusal (DiscreteCostFunction::
    // set_mplp_forbid, DESIGN.md 5.19 "Forbidden entries"; what MSMHIP_MPLP_FORBID=on asks of the executables) -- the strain regulariser produces
    // such entries wherever a label set lets control points meet, as the unscaled sampling grid does
    bool mplp_forbid = false;
    // with pairwise (an extension; what --dopt=MPLP with --regoption=1 asks for under MSMHIP_MPLP=on and MSMHIP_MPLP_PAIRS=on): the pairwise model is
    // solved by MPLP over its unary and pair tables, mciters sweeps per iteration from the zero labelling, both tables on the device (DiscreteCostFunction::
    // mplp_pairs_optimise), in the stand-in solve's place; with mplp_round, mplp_polish polish passes of the winner follow.  mplp_forbid
    // does not apply to it
    bool mplp_pairs = false;
    // the MCMC branch leaves both tables on the device and runs the sweeps there (msm_cost_mcmc_optimise) instead of fetching them for the host
    // optimiser: the same labelings, bit for bit (what MSMHIP_MCMC=gpu asks of the executables)
    bool mcmc_gpu = false;
    // with mcmc_gpu: those sweeps take their proposals from the draw kernel instead of the host's stream (Context::set_mcmc_draw on the level's context):
    // the same proposals, bit for bit (what MSMHIP_MCMC_DRAW=gpu asks of the executables)
    bool mcmc_draw_gpu = false;
    // the MCMC branch runs this many chains per iteration from the one labelling (chain k seeded with seed + it + 1000003 k) and keeps the one with the
    // lowest energy (msm_cost_mcmc_optimise_chains with mcmc_gpu, msm_mcmc_optimise_chains without: the same labelling); 1: the single run
    int mcmc_chains = 1;
    // the level's features for both data sets through one msm_level_features call (level_features_batch: the masked list surgery and create_exclusion on
    // the device) instead of the chain of calls of level_features / finish_features: the same bytes (what MSMHIP_FEATURES=gpu asks of the executables)
    bool features_gpu = false;
    // true: --regoption=1 as --dopt=FastPD drives it (M/mesh_registration.cpp:182-188): the model lists pairs instead of triplets, per iteration
    // computeUnaryCosts + computePairwiseCosts, then a stand-in for FPD::FastPD(model, 100) (msm_pairwise_icm)
    bool pairwise = false;
    int anat_order = -1;  // --anatgrid of this level (regularisermode 4 / 5, aMSM); cp_order + 2 when negative
    // the fusion loop queues the next label step's evaluations while the host solves the current one (msm_cost_triplet_octets_prefetch: a hint, the
    // results do not depend on it)
    bool speculate = true;
    // measurement only: when set, the cost function records HIP events around its kernels (msm_cost_enable_timing) and the duration of every fusion
    // move's kernel (ms) is appended here -- one event query per move, so a run with this set is not the one whose wall clock is reported
    std::vector<double> *move_kernel_ms = nullptr;
};

// the anatomical surfaces of a --regoption=5 (aMSM) run: V x 3 on the vertices of the input / reference SPHERE (MESHES[0] / MESHES[1]), whose handles
// the level loop searches (set_anatomical, M/mesh_registration.cpp:437-441)
struct Anatomy {
    Mesh *in_sphere = nullptr, *ref_sphere = nullptr;
    const Points *in_anat = nullptr, *ref_anat = nullptr;
};

// --inweight / --refweight brought to a level's data grid (downsample_cfweighting, M/mesh_registration.cpp:334-350: nearest neighbour): rows x V(data grid)
struct Weighting {
    const Matrix *in_weight = nullptr, *ref_weight = nullptr;
    int in_rows = 0, ref_rows = 0;
};

// Mesh_registration::combine_costfunction_weighting, M/mesh_registration.cpp:849-869: the mean of the two weightings over the rows both have; the rows
// only the larger one has are kept.  a: ra x V, b: rb x V.
inline Matrix combine_costfunction_weighting(const Matrix &a, int ra, const Matrix &b, int rb, int *rows) {
    Matrix out = ra >= rb ? a : b;
    const size_t V = ra > 0 ? a.size() / (size_t)ra : 0, n = (size_t)std::min(ra, rb) * V;
    for (size_t i = 0; i < n; ++i) out[i] = (a[i] + b[i]) / 2.0;
    *rows = std::max(ra, rb);
    return out;
}

struct LevelResult {
    Points sph_reg, cpgrid;
    std::vector<double> energies;
    std::vector<std::vector<int32_t>> labelings;
};

// m_CPgrid.set_coord(i, m_ROT[i] * m_labels[labeling[i]]), operator*(Matrix, Point) R/point.cpp:207-213
inline Points apply_labeling(const std::vector<double> &ROT, const Points &labels, const std::vector<int32_t> &labeling) {
    const size_t N = labeling.size();
    Points out(3 * N);
    for (size_t i = 0; i < N; ++i) {
        const double *R = &ROT[9 * i], *v = &labels[3 * (size_t)labeling[i]];
        for (int r = 0; r < 3; ++r) out[3 * i + r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2];
    }
    return out;
}

// target / source: the reference and the moving sphere at this level's data resolution with their D x V features;
// sph_reg: the current registered position of the source sphere; cp_start: the control grid after warp_CPgrid, or null
inline LevelResult run_discrete_opt(Context &ctx, const Points &target_xyz, const Triangles &target_tri, const Matrix &ref_feat,
                                    const Points &source_xyz, const Triangles &source_tri, const Matrix &src_feat, int D, Points sph_reg,
                                    int cp_order, const LevelOptions &o, const Points *cp_start = nullptr, PhaseClock *clock = nullptr,
                                    const Anatomy *anat = nullptr, const Weighting *weights = nullptr) {
    // ---- initialize_level / Initialize(CONTROL)
    auto [cp_xyz, cp_tri] = make_mesh_from_icosa(cp_order);
    Mesh TARGET(ctx, target_xyz, target_tri), SOURCE(ctx, source_xyz, source_tri), CPGRID(ctx, cp_xyz, cp_tri);
    TARGET.set_pvalues(ref_feat);
    auto [MAXSEP, MVDmax] = cp_spacings(cp_xyz, cp_tri);
    auto [samples, barycentres] = label_sampling_grid(o.sg_order < 0 ? cp_order + 2 : o.sg_order, o.labeldist * MVDmax);
    const double centre[3] = {samples[0], samples[1], samples[2]};
    if (o.pairwise && o.cost.regularisermode != 1) throw Error(MSM_ERR_INVALID, "MeshREG ERROR:: you cannot run higher order clique regularisers with fastPD ");
    const std::vector<int32_t> triplets = o.pairwise ? std::vector<int32_t>() : estimate_triplets(cp_tri);
    const std::vector<int32_t> pairs = o.pairwise ? estimate_pairs(cp_tri, (int)(cp_xyz.size() / 3)) : std::vector<int32_t>();
    if (o.mcmc_draw_gpu) {
        if (!o.mcmc_gpu) throw Error(MSM_ERR_INVALID, "LevelOptions: mcmc_draw_gpu draws the proposals of the GPU sweeps: it needs mcmc_gpu");
        ctx.set_mcmc_draw(1);
    }
    DiscreteCostFunction costfct(ctx, o.cost);
    costfct.set_meshes(TARGET, SOURCE, CPGRID);  // _ORIG, _oCPgrid
    costfct.set_featurespace(src_feat, D);
    if (o.mplp_forbid) costfct.set_mplp_forbid(true);
    costfct.set_spacings(MAXSEP, MVDmax);
    std::unique_ptr<Mesh> anat_sphere;
    if (o.cost.regularisermode == 4 || o.cost.regularisermode == 5) {  // initialize_level, M/mesh_registration.cpp:91-104
        if (o.cost.regularisermode == 4)
            throw Error(MSM_ERR_INVALID, "--regoption 4 has been removed from newMSM. Use --regoption 3 for spherical mesh regularisation or --regoption 5 for "
                                         "anatomical mesh regularisation.");
        if (!anat || !anat->in_sphere || !anat->ref_sphere || !anat->in_anat || !anat->ref_anat)
            throw Error(MSM_ERR_INVALID, "--regoption 5 requires anatomical meshes. Use --regoption 3 for spherical mesh regularisation or provide anatomical meshes.");
        if (o.pairwise) throw Error(MSM_ERR_INVALID, "MeshREG ERROR:: you cannot run higher order clique regularisers with fastPD ");
        // resample_anatomy (:250-332): ANAT_ico with NEARESTFACES and _ANATbaryweights, both anatomies resampled onto it
        const AnatomyGrid grid = resample_anatomy_grid(cp_xyz, cp_tri, std::max(0, (o.anat_order < 0 ? cp_order + 2 : o.anat_order) - cp_order));
        const Points anat_orig = PhaseClock::timed(clock, "surface_resample", [&] { return barycentric_coords_resample(*anat->in_sphere, *anat->in_anat, grid.sphere_xyz); });
        const Points anat_target = PhaseClock::timed(clock, "surface_resample", [&] { return barycentric_coords_resample(*anat->ref_sphere, *anat->ref_anat, grid.sphere_xyz); });
        anat_sphere.reset(new Mesh(ctx, grid.sphere_xyz, grid.sphere_tri));
        costfct.setTriplets(triplets);  // NEARESTFACES is indexed by triplet = control triangle
        costfct.set_anatomical(*anat_sphere, anat_target, anat_orig, grid.sphere_tri, grid.weights, grid.face_ptr, grid.face_idx);
    }
    const int N = (int)(cp_xyz.size() / 3);
    if (o.move_kernel_ms) check(msm_cost_enable_timing(costfct.handle(), 1));
    int m_iter = 1;
    double m_scale = 1.0;
    if (cp_start) cp_xyz = *cp_start;
    LevelResult res;
    detail::HostBuffer octets[2];  // used in turn: a step's costs are read by its solve while the next step may already be written into the other
    for (int it = 0; it < o.iters; ++it) {
        // ---- reset_meshspace + setupCostFunction
        SOURCE.set_coords(sph_reg);
        if (weights && weights->in_weight && weights->ref_weight) {  // setupCostFunctionWeighting(combine_weighting()), M/mesh_registration.cpp:171,334-350
            const Matrix resampled = PhaseClock::timed(clock, "metric_resample", [&] { return metric_resample(TARGET, *weights->ref_weight, SOURCE); });
            int rows = 0;
            const Matrix W = combine_costfunction_weighting(*weights->in_weight, weights->in_rows, resampled, weights->ref_rows, &rows);
            costfct.set_dataaffintyweighting(W, rows);
        }
        costfct.reset_source(SOURCE);
        CPGRID.set_coords(cp_xyz);
        costfct.reset_CPgrid(CPGRID);
        const std::vector<double> ROT = cp_rotations(centre, cp_xyz);
        Points labels;
        if (o.rescale_labels) labels = rescale_sampling_grid(samples, m_scale);
        else labels = (m_iter % 2 == 0) ? samples : barycentres;
        costfct.set_labels(labels, ROT);
        PhaseClock::timed(clock, "get_source_data", [&] { costfct.get_source_data(); });
        if (o.pairwise) costfct.setPairs(pairs);
        else costfct.setTriplets(triplets);
        ++m_iter;
        const bool mplp = o.mplp && !o.fusion && !o.pairwise;
        const bool mcmc_gpu = o.mcmc_gpu && !o.fusion && !o.pairwise && !mplp;
        const bool mplp_pairs = o.mplp_pairs && o.pairwise && !o.fusion;
        if (!mcmc_gpu && !mplp && !mplp_pairs) PhaseClock::timed(clock, "unary_table", [&] { costfct.computeUnaryCosts(); });
        std::vector<int32_t> labeling((size_t)N, 0);  // resetLabeling
        const int L = (int)(labels.size() / 3), T = (int)(triplets.size() / 3);
        if (o.fusion) {  // ---- Fusion::optimize: two sweeps over the labels, a fusion move per label step
            double *Ebuf[2] = {octets[0].ensure(ctx.handle(), 8 * (size_t)T), octets[1].ensure(ctx.handle(), 8 * (size_t)T)};  // pinned, GPU-mapped
            int turn = 0;
            std::vector<double> unary2(2 * (size_t)N);
            const std::vector<int32_t> no_pairs;
            auto differs = [&](int label) {
                for (int i = 0; i < N; ++i)
                    if (labeling[(size_t)i] != label) return true;
                return false;
            };
            for (int step = 0; step < 2 * L; ++step) {
                const int label = step % L;
                if (!differs(label)) continue;
                if (o.fusion_mplp) {  // octets, unary gather and the MPLP solve on the device
                    const FusionMplp r = PhaseClock::timed(clock, "optimiser", [&] { return costfct.fusion_mplp_step(labeling, label, o.fusion_sweeps, o.fusion_polish); });
                    for (int i = 0; i < N; ++i)
                        if (r.x[(size_t)i] == 1 && labeling[(size_t)i] != label) labeling[(size_t)i] = label;
                    continue;
                }
                double *E = Ebuf[turn];
                turn ^= 1;
                PhaseClock::timed(clock, "fusion_moves", [&] { check(msm_cost_triplet_octets(costfct.handle(), labeling.data(), label, E)); });
                if (o.move_kernel_ms) {
                    double ms = 0.0;
                    int32_t got = 0;
                    check(msm_cost_kernel_times(costfct.handle(), &ms, 1, &got));
                    if (got == 1) o.move_kernel_ms->push_back(ms);
                }
                if (o.speculate && !o.move_kernel_ms) {  // the next step that will be evaluated if this solve changes nothing: queued while the host solves
                    for (int nxt = step + 1; nxt < 2 * L; ++nxt)
                        if (differs(nxt % L)) {
                            PhaseClock::timed(clock, "fusion_prefetch", [&] { check(msm_cost_triplet_octets_prefetch(costfct.handle(), labeling.data(), nxt % L, Ebuf[turn])); });
                            break;
                        }
                }
                for (int i = 0; i < N; ++i) {
                    unary2[2 * (size_t)i] = costfct.unarycosts[(size_t)labeling[(size_t)i] * N + i];
                    unary2[2 * (size_t)i + 1] = costfct.unarycosts[(size_t)label * N + i];
                }
                const std::vector<int32_t> x =
                    PhaseClock::timed(clock, "optimiser", [&] { return fusion_icm_step(N, unary2, nullptr, no_pairs, E, triplets, o.icm_passes); });
                for (int i = 0; i < N; ++i)
                    if (x[(size_t)i] == 1 && labeling[(size_t)i] != label) labeling[(size_t)i] = label;
            }
        } else if (mplp_pairs) {  // ---- MPLP over the pair tables, tables and sweeps on the device, then the polish of the winner where asked for
            PhaseClock::timed(clock, "optimiser", [&] { costfct.mplp_pairs_optimise(o.mciters, o.mplp_round ? o.mplp_polish : 0, labeling); });
        } else if (o.pairwise) {  // ---- FastPD: computeUnaryCosts, computePairwiseCosts, the solve
            PhaseClock::timed(clock, "pairwise_table", [&] { costfct.computePairwiseCosts(); });
            PhaseClock::timed(clock, "optimiser", [&] { pairwise_icm(costfct.unarycosts, costfct.paircosts, pairs, N, L, labeling, 100); });
        } else if (mplp) {  // ---- MPLP with the tables and the sweeps on the device
            if (o.mplp_round)
                PhaseClock::timed(clock, "optimiser", [&] { costfct.mplp_round(o.mciters, o.mplp_polish, labeling, true); });
            else
                PhaseClock::timed(clock, "optimiser", [&] { costfct.mplp_optimise(o.mciters, labeling); });
        } else if (mcmc_gpu) {  // ---- MCMC with the tables and the sweeps on the device: the labeling of the branch below
            if (o.mcmc_chains > 1)
                PhaseClock::timed(clock, "optimiser", [&] { costfct.mcmc_optimise_chains(o.mcparam, o.mciters, mcmc_chain_seeds(o.seed + (uint64_t)it, o.mcmc_chains), labeling); });
            else
                PhaseClock::timed(clock, "optimiser", [&] { costfct.mcmc_optimise(o.mcparam, o.mciters, o.seed + (uint64_t)it, labeling); });
        } else {  // ---- MCMC: computeUnaryCosts, computeTripletCosts, optimise
            const std::vector<double> tcosts = PhaseClock::timed(clock, "triplet_table", [&] { return costfct.computeTripletCosts(); });
            if (o.mcmc_chains > 1)
                PhaseClock::timed(clock, "optimiser", [&] {
                    mcmc_optimise_chains(costfct.unarycosts, tcosts, triplets, N, L, o.mcparam, o.mciters, mcmc_chain_seeds(o.seed + (uint64_t)it, o.mcmc_chains), labeling);
                });
            else
                PhaseClock::timed(clock, "optimiser", [&] { mcmc_optimise(costfct.unarycosts, tcosts, triplets, N, L, o.mcparam, o.mciters, o.seed + (uint64_t)it, labeling); });
        }
        res.energies.push_back(PhaseClock::timed(clock, "total_cost", [&] { return costfct.evaluateTotalCostSum(labeling); }));
        res.labelings.push_back(labeling);
        // ---- applyLabeling, warp the source through the control grid's move, unfold both (:219-230)
        const Points moved = apply_labeling(ROT, labels, labeling);
        // SOURCE holds sph_reg since the top of the iteration; CPGRID still holds the previous grid
        PhaseClock::timed(clock, "sphere_project_warp", [&] { sphere_project_warp(SOURCE, CPGRID, moved); });
        CPGRID.set_coords(moved);
        PhaseClock::timed(clock, "unfold", [&] { return unfold(CPGRID); });
        cp_xyz = CPGRID.get_coords();
        PhaseClock::timed(clock, "unfold", [&] { return unfold(SOURCE); });
        sph_reg = SOURCE.get_coords();
    }
    res.sph_reg = sph_reg;
    res.cpgrid = cp_xyz;
    return res;
}

// one resolution level of a schedule (msmhip_config.hpp: levels_from_config fills these from a configuration file)
struct LevelSpec {
    int data_order = 5, cp_order = 2;
    double sigma_in = 0.0, sigma_ref = 0.0;
    LevelOptions options;
    // a RIGID level (levels_from_config(..., rigid = true)): Rigid_cost_function with options.iters, options.cost.simmeasure and these
    bool rigid = false;
    double stepsize = (double)0.01f, gradsampling = 0.5;
};

struct MultiresResult {
    Points sphere_reg;                            // the input sphere moved through the final warp ("sphere.reg", M/mesh_registration.cpp:352-356)
    std::vector<Points> level_reg;                // the registered data grid of every level
    std::vector<std::vector<double>> energies;    // per level, per iteration (a RIGID level: its trace, six values per iteration)
    std::vector<std::vector<int32_t>> labelings;  // every iteration's labeling, level after level
};

// --excl / --cutthr: exclusion masks from the cut thresholds in every level's feature preparation (level_features)
struct Exclusion {
    bool on = false;
    double lower = 0.0, upper = 0.0001;  // --cutthr
};

// --IN / --INc (levels_from_config(..., &intensity) opts in): on = _IN, cut = _cut, which --INc alone sets (M/mesh_registration.cpp:694-703)
struct IntensityNorm {
    bool on = false, cut = false;
};

// One data set of featurespace::initialise (M/featurespace.cpp:52-84) on a level's grid `ico`: metric_resample from its native mesh, smooth_data when
// sigma > 0, variance_normalise when varnorm.  With excl.on the mask is create_exclusion of the native data over the cut range (1 = kept, 0 = every
// feature inside it: the medial wall of real data); resampling and smoothing leave it out and each replaces the mask by its own on the grid
// (R/resampler.cpp:54-67, 168-230); the variance statistics run over vertices with mask > 0 and the others stay as they are (M/reg_tools.cpp:804-843).
// Made afresh at every level from the native data, as the reference does.  mask_out (optional): the level-grid mask (empty without excl.on).
inline Matrix level_features(Mesh &mesh, const Matrix &data, Mesh &ico, double sigma, bool varnorm, const Exclusion &excl, PhaseClock *clock,
                             std::vector<double> *mask_out = nullptr) {
    std::vector<double> mask;
    if (excl.on) mask = create_exclusion(data, mesh.nvertices(), excl.lower, excl.upper);
    std::vector<double> *EXCL = excl.on ? &mask : nullptr;
    Matrix f = PhaseClock::timed(clock, "metric_resample", [&] { return metric_resample(mesh, data, ico, EXCL); });
    if (sigma > 0.0) f = PhaseClock::timed(clock, "smooth_data", [&] { return smooth_data(ico, f, ico, sigma, EXCL); });
    if (varnorm) variance_normalise(f, ico.nvertices(), EXCL);
    if (mask_out) *mask_out = std::move(mask);
    return f;
}

// The reference side of every level's feature preparation, prepared once for many registrations against one reference: per level the output of
// level_features for the reference data (resampled, smoothed, variance normalised unless --IN / --INc postpone that) and the level-grid mask.  It depends
// on the reference, the level schedule, --excl / --cutthr and --INc, not on the subject: one cache serves runs that agree in those.  Filled on first use
// and read afterwards; the entries are vectors the cache owns.  One cache serves one thread at a time.
struct ReferenceCache {
    struct Entry {
        bool filled = false;
        Matrix features;
        std::vector<double> mask;
    };
    std::vector<Entry> levels;
    int hits = 0, fills = 0;
};

// The tail of featurespace::initialise (M/featurespace.cpp:75-83) over data sets that level_features has resampled and smoothed (varnorm = false there):
// with inorm.on every data set i >= 1 is histogram matched to data set 0 -- one call, the target's statistics computed once -- with the masks as they stand
// after smoothing (masked: --excl or --INc), then variance_normalise of every data set when varnorm.  The reference's order is a quirk in a pairwise run,
// whose data sets are (input, reference): there the REFERENCE data is matched to the INPUT data.  feats: D x V(ico) each.
inline void finish_features(Context &ctx, std::vector<Matrix> &feats, const std::vector<std::vector<double>> &masks, bool masked, int D, int V,
                            const IntensityNorm &inorm, bool varnorm, PhaseClock *clock) {
    const size_t n = feats.size();
    if (inorm.on && n > 1) {
        Matrix srcs;
        std::vector<double> src_masks;
        for (size_t i = 1; i < n; ++i) {
            srcs.insert(srcs.end(), feats[i].begin(), feats[i].end());
            if (masked) src_masks.insert(src_masks.end(), masks[i].begin(), masks[i].end());
        }
        const Matrix matched = PhaseClock::timed(clock, "histogram_match", [&] {
            return histogram_match(ctx, (int)n - 1, D, V, srcs, V, feats[0], masked ? &src_masks : nullptr, 1, masked ? &masks[0] : nullptr, 1);
        });
        for (size_t i = 1; i < n; ++i) feats[i].assign(matched.begin() + (long)((i - 1) * (size_t)D * V), matched.begin() + (long)(i * (size_t)D * V));
    }
    if (varnorm)
        for (size_t i = 0; i < n; ++i) variance_normalise(feats[i], V, masked ? &masks[i] : nullptr);
}

// project_CPgrid (M/mesh_registration.cpp:131-162) for a level that starts from a warp of the input sphere, in_mesh -> moved_in: the warp of the
// previous level carried to the input sphere (`incurrent`) or, at the first level, the --trans sphere.  The level's data grid is carried through it
// and unfolded; so is its control grid (warp_CPgrid, M/DiscreteModel.h:140-143) when cp_start is given (a rigid level has no control grid).
inline Points project_start(Context &ctx, const Points &ico_xyz, const Triangles &ico_tri, Mesh &in_mesh, const Points &moved_in, int cp_order, Points *cp_start,
                            PhaseClock *clock) {
    Mesh moved(ctx, PhaseClock::timed(clock, "sphere_project_warp", [&] { return sphere_project_warp(ico_xyz, in_mesh, moved_in); }), ico_tri);
    if (cp_start) {
        auto [cp_xyz, cp_tri] = make_mesh_from_icosa(cp_order);
        Mesh cpm(ctx, PhaseClock::timed(clock, "sphere_project_warp", [&] { return sphere_project_warp(cp_xyz, in_mesh, moved_in); }), cp_tri);  // warp_CPgrid
        PhaseClock::timed(clock, "unfold", [&] { return unfold(cpm); });
        *cp_start = cpm.get_coords();
    }
    PhaseClock::timed(clock, "unfold", [&] { return unfold(moved); });
    return moved.get_coords();
}

// The --trans sphere as project_CPgrid looks at it at the first level (M/mesh_registration.cpp:136-145): null when it was not given or has the input
// sphere's coordinates (Mesh operator==, R/mesh.cpp:1285-1290: every coordinate within EPSILON = 1e-8), with the reference's warning.  It is taken as
// it is, not recentred and not rescaled (set_transformed); it must have the input sphere's vertex count, because sphere_project_warp reads it at the
// input sphere's vertex numbers (the reference would read out of bounds).
inline const Points *usable_transformed(const Points *trans_xyz, const Points &in_xyz) {
    if (!trans_xyz) return nullptr;
    if (trans_xyz->size() != in_xyz.size())
        throw Error(MSM_ERR_INVALID, "MeshREG ERROR:: the transformed mesh (--trans) has " + std::to_string(trans_xyz->size() / 3) + " vertices, the input mesh has " +
                                         std::to_string(in_xyz.size() / 3));
    for (size_t i = 0; i < in_xyz.size(); ++i)
        if (!(std::fabs((*trans_xyz)[i] - in_xyz[i]) < 1e-8)) return trans_xyz;
    std::cerr << " WARNING: transformed mesh has the same coordinates as the input mesh " << std::endl;
    return nullptr;
}

inline const char *excl_with_weightings_message() {
    return "--excl together with --inweight and --refweight is not available: downsample_cfweighting (M/mesh_registration.cpp:334-350) reads the level grid's "
           "exclusion mask at vertex numbers of the weightings' own meshes, which is out of bounds or meaningless unless the two meshes have the same size";
}

// Mesh_registration::run_multiresolutions (M/mesh_registration.cpp:30-50) for DISCRETE and RIGID levels without file I/O -- the C++ twin of
// newmsm_amd/registration.py: run_multiresolution (same calls in the same order; tests/test_cpp_host.py compares the two):
//   per level  featurespace::initialise (M/featurespace.cpp:39-86: metric_resample of both data sets onto the level's icosphere, smooth_data,
//              variance_normalise), project_CPgrid (M/mesh_registration.cpp:131-162: the warp of the previous level carried to the new data
//              grid and control grid, unfold) and run_discrete_opt;
//   at the end transform (:352-356).
// A RIGID level runs Rigid_cost_function on the level's featurespace instead of run_discrete_opt (:66-72, 112-116): no control grid, no labelings.
// in_* / ref_*: the input and reference spheres (radius 100) with their D x V data.
// trans_xyz (--trans, optional): the input sphere as an earlier registration left it (its sphere.reg), taken as it is.  Only the first level looks at
// it: its data grid and control grid start carried through input sphere -> trans_xyz, which is what every later level does with the warp of the level
// before it, so sphere_reg is the composition.  A first level that is RIGID has no control grid to carry (the reference would call warp_CPgrid on a
// model that does not exist yet); its data grid is projected.
// excl (--excl, --cutthr): masks in the feature preparation only.  They do not enter the cost function: combine_weighting (:234-248) returns ones
// unless both weightings are given, and that combination is refused (excl_with_weightings_message).
// inorm (--IN / --INc): in every level's feature preparation, RIGID levels included, the reference data is histogram matched to the input data after both
// are resampled and smoothed and before variance normalisation (finish_features); inorm.cut makes the masks exist as --excl does (M/featurespace.cpp:61).
// The final resampling is the caller's (transformed_data).
// ref_cache (optional): the reference data's level_features output is taken from it, and put there by the first run that needs it, instead of being
// computed at every level of every run; everything after it (finish_features, the level's target mesh) stays this run's own.  Without it every call is
// what it was before the argument existed.
inline MultiresResult run_multiresolutions(Context &ctx, const Points &in_xyz, const Triangles &in_tri, const Matrix &in_data, const Points &ref_xyz,
                                           const Triangles &ref_tri, const Matrix &ref_data, int D, const std::vector<LevelSpec> &levels, bool varnorm,
                                           PhaseClock *clock = nullptr, const Points *in_anat = nullptr, const Points *ref_anat = nullptr,
                                           const Matrix *in_cfweight = nullptr, int in_cfrows = 0, const Matrix *ref_cfweight = nullptr, int ref_cfrows = 0,
                                           const Points *trans_xyz = nullptr, const Exclusion &excl = Exclusion(), const IntensityNorm &inorm = IntensityNorm(),
                                           ReferenceCache *ref_cache = nullptr) {
    if (levels.empty()) throw Error(MSM_ERR_INVALID, "run_multiresolutions: no DISCRETE level");
    if ((in_anat != nullptr) != (ref_anat != nullptr)) throw Error(MSM_ERR_INVALID, "Error: must supply both anatomical meshes or none");  // CLI/newmsm.cpp:41-43
    if (in_anat && (in_anat->size() != in_xyz.size() || ref_anat->size() != ref_xyz.size()))
        throw Error(MSM_ERR_INVALID, "MeshREG ERROR:: input/reference anatomical mesh resolution is inconsistent with input/reference spherical mesh resolution.");
    if (excl.on && in_cfweight && ref_cfweight) throw Error(MSM_ERR_INVALID, excl_with_weightings_message());
    trans_xyz = usable_transformed(trans_xyz, in_xyz);
    Mesh in_mesh(ctx, in_xyz, in_tri), ref_mesh(ctx, ref_xyz, ref_tri);
    Anatomy anatomy;
    if (in_anat) anatomy.in_sphere = &in_mesh, anatomy.ref_sphere = &ref_mesh, anatomy.in_anat = in_anat, anatomy.ref_anat = ref_anat;
    MultiresResult res;
    Points sph_reg_prev;
    int prev_order = -1;
    if (ref_cache && ref_cache->levels.size() < levels.size()) ref_cache->levels.resize(levels.size());
    size_t li = 0;
    for (const LevelSpec &lv : levels) {
        auto [ico_xyz, ico_tri] = make_mesh_from_icosa(lv.data_order);
        Mesh ico(ctx, ico_xyz, ico_tri);
        std::vector<Matrix> feats(2);
        std::vector<std::vector<double>> masks(2);
        const bool postponed = inorm.on || inorm.cut;  // resample and smooth only: matching and variance normalisation follow when both data sets are there
        Exclusion masked = excl;
        masked.on = excl.on || (postponed && inorm.cut);
        ReferenceCache::Entry *entry = ref_cache ? &ref_cache->levels[li] : nullptr;
        ++li;
        bool finish = postponed;
        if (lv.options.features_gpu) {  // featurespace::initialise in one call (msm_level_features): the bytes of the loop below
            const auto batch = [&](const std::vector<Mesh *> &m, const std::vector<const Matrix *> &d, const std::vector<double> &s, bool match, bool vn) {
                return PhaseClock::timed(clock, "level_features", [&] { return level_features_batch(ico, m, d, D, s, masked.on, match, vn, masked.lower, masked.upper); });
            };
            if (!entry) {
                feats = batch({&in_mesh, &ref_mesh}, {&in_data, &ref_data}, {lv.sigma_in, lv.sigma_ref}, inorm.on, varnorm).features;
                finish = false;
            } else {  // the input data alone; the reference's from the cache, which one call of its own fills; the tail over the two as below
                LevelFeatures one = batch({&in_mesh}, {&in_data}, {lv.sigma_in}, false, postponed ? false : varnorm);
                feats[0] = std::move(one.features[0]), masks[0] = std::move(one.masks[0]);
                if (entry->filled) {
                    ++ref_cache->hits;
                } else {
                    one = batch({&ref_mesh}, {&ref_data}, {lv.sigma_ref}, false, postponed ? false : varnorm);
                    entry->features = std::move(one.features[0]), entry->mask = std::move(one.masks[0]), entry->filled = true;
                    ++ref_cache->fills;
                }
                feats[1] = entry->features, masks[1] = entry->mask;
            }
        }
        for (int k = 0; k < 2 && !lv.options.features_gpu; ++k) {
            if (k == 1 && entry && entry->filled) {
                feats[1] = entry->features, masks[1] = entry->mask;
                ++ref_cache->hits;
                continue;
            }
            feats[(size_t)k] = level_features(k == 0 ? in_mesh : ref_mesh, k == 0 ? in_data : ref_data, ico, k == 0 ? lv.sigma_in : lv.sigma_ref,
                                              postponed ? false : varnorm, masked, clock, &masks[(size_t)k]);
            if (k == 1 && entry) {
                entry->features = feats[1], entry->mask = masks[1], entry->filled = true;
                ++ref_cache->fills;
            }
        }
        if (finish) finish_features(ctx, feats, masks, masked.on, D, ico.nvertices(), inorm, varnorm, clock);
        // project_CPgrid: the warp this level starts from, as the input sphere moved through it -- the previous level's, or --trans at the first
        Points sph_in, cp_start, incurrent;
        const Points *moved_in = trans_xyz;
        if (!sph_reg_prev.empty()) {
            auto [prev_xyz, prev_tri] = make_mesh_from_icosa(prev_order);
            Mesh prev(ctx, prev_xyz, prev_tri);
            incurrent = PhaseClock::timed(clock, "sphere_project_warp", [&] { return sphere_project_warp(in_xyz, prev, sph_reg_prev); });
            moved_in = &incurrent;
        }
        const bool have_cp_start = moved_in && !lv.rigid;  // (a rigid level has no control grid: no warp_CPgrid)
        if (moved_in) {
            sph_in = project_start(ctx, ico_xyz, ico_tri, in_mesh, *moved_in, lv.cp_order, have_cp_start ? &cp_start : nullptr, clock);
        } else {  // level 1, no transformed mesh: project_CPgrid only unfolds the (regular) data grid
            Mesh moved(ctx, ico_xyz, ico_tri);
            PhaseClock::timed(clock, "unfold", [&] { return unfold(moved); });
            sph_in = moved.get_coords();
        }
        if (lv.rigid) {
            Points reg = PhaseClock::timed(clock, "rigid", [&] {
                RigidCostFunction rcf(ctx, ico, ico, feats[0], feats[1], D, lv.options.cost.simmeasure);
                rcf.initialise();
                rcf.update_source(sph_in);
                std::vector<double> trace;
                Points out = rcf.run(lv.options.iters, lv.stepsize, lv.gradsampling, &trace);
                res.energies.push_back(std::move(trace));
                return out;
            });
            res.level_reg.push_back(reg);
            sph_reg_prev = std::move(reg);
            prev_order = lv.data_order;
            continue;
        }
        Matrix w_in, w_ref;
        Weighting weights;
        if (in_cfweight && ref_cfweight) {  // downsample_cfweighting: both weightings onto the level's data grid by nearest neighbour
            w_in = nearest_neighbour_interpolation(in_mesh, *in_cfweight, ico_xyz);
            w_ref = nearest_neighbour_interpolation(ref_mesh, *ref_cfweight, ico_xyz);
            weights.in_weight = &w_in, weights.ref_weight = &w_ref, weights.in_rows = in_cfrows, weights.ref_rows = ref_cfrows;
        }
        LevelResult r = run_discrete_opt(ctx, ico_xyz, ico_tri, feats[1], ico_xyz, ico_tri, feats[0], D, sph_in, lv.cp_order, lv.options,
                                         have_cp_start ? &cp_start : nullptr, clock, in_anat ? &anatomy : nullptr, in_cfweight && ref_cfweight ? &weights : nullptr);
        res.labelings.insert(res.labelings.end(), r.labelings.begin(), r.labelings.end());
        res.energies.push_back(r.energies);
        res.level_reg.push_back(r.sph_reg);
        sph_reg_prev = std::move(r.sph_reg);
        prev_order = lv.data_order;
    }
    auto [last_xyz, last_tri] = make_mesh_from_icosa(levels.back().data_order);
    Mesh last(ctx, last_xyz, last_tri);
    res.sphere_reg = PhaseClock::timed(clock, "sphere_project_warp", [&] { return sphere_project_warp(in_xyz, last, sph_reg_prev); });
    return res;
}

// save_transformed_data without its file I/O (M/mesh_registration.cpp:358-395): the native input data resampled from the registered input sphere `moved`
// onto the reference sphere.  excl.on: fresh masks from the native data keep the cut out of the resampling (:371-375).  inorm.on: the native input data is
// first histogram matched to the native reference data (:376-380) -- this way round here, unlike in the levels' feature preparation -- with those masks
// under --excl only (--INc's cut alone makes none here).
inline Matrix transformed_data(Context &ctx, Mesh &moved, const Matrix &in_data, Mesh &target, const Matrix &ref_data, int D, const Exclusion &excl = Exclusion(),
                               const IntensityNorm &inorm = IntensityNorm()) {
    std::vector<double> in_excl;
    if (excl.on) in_excl = create_exclusion(in_data, moved.nvertices(), excl.lower, excl.upper);
    if (!inorm.on) return metric_resample(moved, in_data, target, excl.on ? &in_excl : nullptr);
    std::vector<double> ref_excl;
    if (excl.on) ref_excl = create_exclusion(ref_data, target.nvertices(), excl.lower, excl.upper);
    const Matrix matched = histogram_match(ctx, 1, D, moved.nvertices(), in_data, target.nvertices(), ref_data, excl.on ? &in_excl : nullptr, 1,
                                           excl.on ? &ref_excl : nullptr, 1);
    return metric_resample(moved, matched, target, excl.on ? &in_excl : nullptr);
}

}  // namespace msmhip

#endif
