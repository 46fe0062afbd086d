// msmhip_dedrift.hpp -- dedrifting and the group statistics of a finished groupwise run in C++ (header only, C++17, no HIP headers), over the
// msm_dedrift_* entry points of msmhip.h: the call sequence of newmsm_amd/dedrift.py: dedrift_group, so that both hosts make the same library calls
// in the same order and get the same bits.
//
// What it replaces: the wb_command / nibabel part of the reference's tutorial pipeline after gMSM (gMSM_scripts/gMSM_tutorial/gw_MSM.sh:65-128,
// compare_stats.py).  Per subject s: orig = M_s, its input sphere as the run used it; reg = R_s, its registered sphere (same triangles); data = F_s.
//   inverse_s    the template's vertices located on R_s, their weights applied to M_s (project_anatomical_mesh's sum; the tutorial unprojects to the
//                template itself, which is the same thing exactly when M_s is the template)
//   W            the mean of the inverses in subject order, minus the midpoint of its bounding box, scaled to radius 100
//   corrected_s  sphere_project_warp(R_s, T, W);  resampled_s  metric_resample(F_s: corrected_s -> T);  distortion_s  log2 J, log2 R per vertex
//   mean / stdev over the subjects (population form), cc / dice per pair of subjects and feature
// Points are AoS and matrices row-major, as everywhere in msmhip.hpp; errors are thrown as msmhip::Error.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "msmhip.hpp"

namespace msmhip {

struct DedriftSubject {
    Points orig, reg;  // M_s and R_s
    Triangles tri;
    Matrix data;       // D x V_s
};

struct DedriftResult {
    int S = 0, D = 0, Vt = 0;
    Points W, drift;                                // the dedrift warp and the drift it comes from, V(T) points each
    std::vector<Points> corrected;                  // per subject
    std::vector<Matrix> resampled, distortion;      // per subject: D x V(T); 2 x V_s (row 0 areal, row 1 shape)
    Matrix mean, stdev;                             // D x V(T)
    Matrix cc, dice;                                // D x S x S
    std::vector<double> cc_mean, dice_mean;         // per feature: the mean over the pairs i < j
    double areal_mean = 0, areal_max = 0, areal_95 = 0, areal_98 = 0, shape_mean = 0, shape_max = 0;  // compare_stats.py:71-105
};

// msm_dedrift: one group on one template
class Dedrift {
public:
    Dedrift(Context &ctx, Mesh &template_mesh, int num_subjects) : S_(num_subjects), Vt_(template_mesh.nvertices()) {
        h_ = msm_dedrift_create(ctx.handle(), template_mesh.handle(), num_subjects);
        if (!h_) throw Error(MSM_ERR_INVALID, msm_last_error());
    }
    ~Dedrift() { msm_dedrift_destroy(h_); }
    Dedrift(const Dedrift &) = delete;
    Dedrift &operator=(const Dedrift &) = delete;
    void reset() { check(msm_dedrift_reset(h_)); }
    // gw_MSM.sh:76-87: one subject's inverse into the running sum (the order of the calls is the order of the additions)
    void accumulate(Mesh &reg, const Points &orig) {
        check(msm_dedrift_accumulate(h_, reg.handle(), to_soa(orig).data(), (int32_t)(orig.size() / 3), nullptr, nullptr, nullptr));
    }
    // gw_MSM.sh:82-92: W (and the drift)
    Points finish(Points *drift = nullptr) {
        std::vector<double> w(3 * (size_t)Vt_), d(3 * (size_t)Vt_);
        check(msm_dedrift_finish(h_, w.data(), drift ? d.data() : nullptr));
        if (drift) *drift = to_aos(d);
        return to_aos(w);
    }
    // gw_MSM.sh:94-128 for one subject; `reg` holds corrected_s afterwards
    void correct(int subject, Mesh &reg, const Points &orig, const Matrix &data, Points &corrected, Matrix &resampled, Matrix &distortion) {
        const int32_t V = (int32_t)(orig.size() / 3), D = (int32_t)(data.size() / (size_t)V);
        std::vector<double> c(3 * (size_t)V);
        resampled.assign((size_t)D * Vt_, 0.0);
        distortion.assign(2 * (size_t)V, 0.0);
        check(msm_dedrift_correct(h_, subject, reg.handle(), to_soa(orig).data(), V, data.data(), D, c.data(), resampled.data(), distortion.data(), nullptr,
                                  nullptr));
        corrected = to_aos(c);
        D_ = D;
    }
    void set_map(int subject, const Matrix &map) {
        D_ = (int)(map.size() / (size_t)Vt_);
        check(msm_dedrift_set_map(h_, subject, map.data(), D_));
    }
    // gw_MSM.sh:108-119, compare_stats.py:12-69
    void group_stats(double percentile, Matrix &mean, Matrix &stdev, Matrix &cc, Matrix &dice) {
        mean.assign((size_t)D_ * Vt_, 0.0);
        stdev.assign((size_t)D_ * Vt_, 0.0);
        cc.assign((size_t)D_ * S_ * S_, 0.0);
        dice.assign((size_t)D_ * S_ * S_, 0.0);
        check(msm_dedrift_group_stats(h_, percentile, mean.data(), stdev.data(), cc.data(), dice.data()));
    }
    // run_cgMSM_ver_gw_iter.sh:171-192: W (V(T) points, a deformation of the template's vertices) replaces the handle's warp as it is; correct may follow
    // without accumulate / finish, and the warp may be replaced between subjects
    void set_warp(const Points &W) { check(msm_dedrift_set_warp(h_, to_soa(W).data())); }
    // run_cgMSM_ver_gw_iter.sh:194-218, extract_info.py: group_stats over the listed resident subjects (in the list's order) and the template vertices
    // with mask > 0 (an empty mask keeps all); cc, dice: D x n x n; cc_mean, dice_mean: per feature the mean over the pairs a < b, from the device
    void group_stats_select(const std::vector<int32_t> &subjects, const std::vector<double> &mask, double percentile, Matrix &mean, Matrix &stdev, Matrix &cc,
                            Matrix &dice, std::vector<double> &cc_mean, std::vector<double> &dice_mean) {
        const size_t n = subjects.size();
        mean.assign((size_t)D_ * Vt_, 0.0);
        stdev.assign((size_t)D_ * Vt_, 0.0);
        cc.assign((size_t)D_ * n * n, 0.0);
        dice.assign((size_t)D_ * n * n, 0.0);
        cc_mean.assign(D_, 0.0);
        dice_mean.assign(D_, 0.0);
        check(msm_dedrift_group_stats_select(h_, subjects.data(), (int32_t)n, mask.empty() ? nullptr : mask.data(), percentile, mean.data(), stdev.data(),
                                             cc.data(), dice.data(), cc_mean.data(), dice_mean.data()));
    }
    int subjects() const { return S_; }
    int rows() const { return D_; }

private:
    msm_dedrift *h_ = nullptr;
    int S_, Vt_, D_ = 0;
};

// the mean over the pairs i < j of each of the D matrices (S x S), summed in the order of compare_stats.py's loops
inline std::vector<double> pair_means(const Matrix &m, int D, int S) {
    std::vector<double> out(D);
    for (int d = 0; d < D; ++d) {
        double acc = 0.0;
        for (int i = 0; i < S; ++i)
            for (int j = i + 1; j < S; ++j) acc += m[((size_t)d * S + i) * S + j];
        out[d] = acc / (S * (S - 1) / 2.0);
    }
    return out;
}

// numpy.percentile, method "linear", of values that are sorted already
inline double percentile_sorted(const std::vector<double> &v, double p) {
    const double vidx = (double)(v.size() - 1) * (p / 100.0), fl = std::floor(vidx), t = vidx - fl;
    const size_t k = (size_t)fl;
    const double a = v[k], b = v[std::min(k + 1, v.size() - 1)], diff = b - a;
    return t >= 0.5 ? b - diff * (1 - t) : a + diff * t;
}

// the whole stage, as newmsm_amd/dedrift.py: dedrift_group runs it
inline DedriftResult dedrift_group(Context &ctx, const Points &template_xyz, const Triangles &template_tri, const std::vector<DedriftSubject> &subjects,
                                   double percentile = 75.0) {
    DedriftResult r;
    const int S = (int)subjects.size();
    Mesh tmpl(ctx, template_xyz, template_tri);
    Dedrift d(ctx, tmpl, S);
    std::vector<std::unique_ptr<Mesh>> regs;
    for (const DedriftSubject &s : subjects) {  // subject order
        regs.emplace_back(new Mesh(ctx, s.reg, s.tri));
        d.accumulate(*regs.back(), s.orig);
    }
    r.W = d.finish(&r.drift);
    r.corrected.resize(S), r.resampled.resize(S), r.distortion.resize(S);
    for (int s = 0; s < S; ++s) {
        d.correct(s, *regs[s], subjects[s].orig, subjects[s].data, r.corrected[s], r.resampled[s], r.distortion[s]);
        regs[s].reset();
    }
    d.group_stats(percentile, r.mean, r.stdev, r.cc, r.dice);
    r.S = S, r.D = d.rows(), r.Vt = tmpl.nvertices();
    r.cc_mean = pair_means(r.cc, r.D, S);
    r.dice_mean = pair_means(r.dice, r.D, S);
    std::vector<double> areal, shape;
    for (const Matrix &m : r.distortion) {
        const size_t V = m.size() / 2;
        for (size_t i = 0; i < V; ++i) areal.push_back(std::fabs(m[i])), shape.push_back(std::fabs(m[V + i]));
    }
    std::sort(areal.begin(), areal.end());
    std::sort(shape.begin(), shape.end());
    double sa = 0, ss = 0;
    for (double v : areal) sa += v;
    for (double v : shape) ss += v;
    r.areal_mean = sa / areal.size(), r.areal_max = areal.back(), r.areal_95 = percentile_sorted(areal, 95), r.areal_98 = percentile_sorted(areal, 98);
    r.shape_mean = ss / shape.size(), r.shape_max = shape.back();
    return r;
}

}  // namespace msmhip
