// resample.hpp -- the adaptive-barycentric resampler (Resampler::get_adaptive_barycentric_weights R/resampler.cpp:72-140 and
// barycentric_data_interpolation :30-70): its host side (resample.cpp) and the launchers of its kernels (resample_kernels.hip).
#pragma once

#include "internal.hpp"

namespace msm {

struct WeightEntry {
    int key;
    double w;
};

// a std::map<int,double> holding the three weights of one query: ascending key, later writes win.  The one definition: the kernels, the host surgery
// (the masked path) and the plan's barycentric rows are bit-identical because they share it.
__host__ __device__ __forceinline__ int small_map(const int *__restrict__ vid, const double *__restrict__ w, int stride, int k, WeightEntry out[3]) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int key = vid[(size_t)j * stride + k];
        const double wt = w[(size_t)j * stride + k];
        int pos = 0;
        while (pos < n && out[pos].key < key) ++pos;
        if (pos < n && out[pos].key == key) {
            out[pos].w = wt;
            continue;
        }
        for (int q = n; q > pos; --q) out[q] = out[q - 1];
        out[pos] = WeightEntry{key, wt};
        ++n;
    }
    return n;
}

// ---- the list surgery on the device (resample_kernels.hip)
struct AdaptiveDevArgs {
    int nOld, nNew;
    const int *fvid, *rvid;        // forward (new -> old) / reverse (old -> new) hit-triangle vertex ids, 3 x N SoA
    const double *fw, *rw;         // their projected barycentric weights
    const double *oldA, *newA;     // vertex areas
    // the counters, one block that the launcher zeroes with one memset: roff | rfill | coff | cfill | long_flag, each B problems long
    int *roff, *rfill, *rkey;      // transposed reverse lists: offsets (nNew + 1), fill counters (nNew), old vertex ids (3 nOld)
    double *rwt;
    int *coff, *cfill, *ckey;      // columns of the result: offsets (nOld + 1), fill counters (nOld), new vertex ids (3 nNew + 3 nOld)
    double *cval, *correction;     // (nOld)
    int *scan_tmp;                 // scratch of the prefix sums, max(nNew, nOld) / 4096 + 2
    int *long_flag;                // 2 per problem: does any transposed reverse list / any column exceed the short sort's limit?
    int *tkey;                     // scratch of the long-list sort, 3 nNew + 3 nOld
    double *tval;
    int *row_ptr, *col;            // the result as CSR: nNew + 1, 3 nNew + 3 nOld
    double *val;
    // an exclusion mask (one problem only; msm_level_features): closest[k] = the old vertex closest to new vertex k, excl: the mask on the old mesh
    // (0 = excluded).  excl == nullptr: no mask, every row takes part
    const int *closest = nullptr;
    const double *excl = nullptr;
    // B problems at once (gMSM: a subject's data mesh rotated to every label against the one template): problem b = blockIdx.y of
    // every launch uses the arrays b * stride elements further on.  fstride / rstride: distance between the three components of
    // fvid / fw and rvid / rw (B * nNew and B * nOld).
    int B = 1;
    size_t fstride = 0, rstride = 0;
    size_t s_f = 0, s_r = 0, s_oldA = 0, s_newA = 0, s_roff = 0, s_rfill = 0, s_r3 = 0, s_coff = 0, s_cfill = 0, s_cap = 0, s_corr = 0, s_rowptr = 0, s_scan = 0;
};
// The device buffers of B simultaneous surgeries (new mesh shared, B old meshes over one triangle list), grow only: a smaller problem reuses the larger
// buffers, and its strides come from its own sizes.  The only place that knows how large each array of AdaptiveDevArgs is.
struct SurgeryScratch {
    DevBuf<int> fvid, rvid, counters, rkey, ckey, row_ptr, col, tkey, scan_tmp;
    DevBuf<double> fw, rw, oldA, newA, ta, rwt, cval, correction, val, tval;  // newA: one set, shared by the problems; ta: B x max(Told, Tnew), scratch of the areas
    int ensure(int nOld, int nNew, int Told, int Tnew, int B);
    AdaptiveDevArgs args(int nOld, int nNew, int B) const;
};
// vertex areas of B coordinate sets over one triangle list: component c of vertex i of set b at xyz[c * comp + b * set + i];
// ta: scratch, B x T; area: B x V
int launch_vertex_areas_batch(msm_ctx *ctx, const double *d_xyz, size_t comp, size_t set, int V, const int32_t *d_tri, int T, const int32_t *d_tid_ptr, const int32_t *d_tid,
                              int B, double *d_ta, double *d_area);
int launch_vertex_areas(msm_ctx *ctx, const double *d_xyz, int V, const int32_t *d_tri, int T, const int32_t *d_tid_ptr, const int32_t *d_tid, double *d_ta,
                        double *d_area);
int launch_adaptive_surgery(msm_ctx *ctx, const AdaptiveDevArgs &a);  // a: from SurgeryScratch::args
// out[b][d][k] = problem b's weights applied to data (D x nOld, shared by the problems); out: B blocks of out_stride doubles
int launch_apply_rows_batch(msm_ctx *ctx, const AdaptiveDevArgs &a, int D, const double *d_data, double *d_out, size_t out_stride);
int launch_apply_rows(msm_ctx *ctx, int nNew, int nOld, int D, const int *row_ptr, const int *col, const double *val, const double *d_data, double *d_out);
// the same with the old mesh's mask d_excl: excluded columns left out, and d_excl_out (nNew) = the rows applied to the mask itself over the kept columns
int launch_apply_rows_masked(msm_ctx *ctx, int nNew, int nOld, int D, const int *row_ptr, const int *col, const double *val, const double *d_data,
                             const double *d_excl, double *d_out, double *d_excl_out);

// ---- the weights of one (in_mesh -> new_mesh) pair (resample.cpp)
// queries AND list surgery on the device (no exclusion mask): the CSR stays in HBM
struct AdaptiveDev {
    int nOld = 0, nNew = 0;
    const int *row_ptr = nullptr, *col = nullptr;  // device; valid until the next adaptive_weights_dev on this context
    const double *val = nullptr;
};
int adaptive_weights_dev(msm_mesh *in_mesh, msm_mesh *new_mesh, AdaptiveDev &out, bool check = true);  // check = false: the caller checks the status word
// the same under an exclusion mask that lies in HBM (d_excl: V(in_mesh) values, 0 = excluded): the closest-vertex search and the masked surgery are queued
// behind the queries, nothing is waited for and the status word is the caller's to check.  Both meshes belong to one context.
int adaptive_weights_dev_masked(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *d_excl, AdaptiveDev &out);
// grows the context's surgery scratch to what a pair of these sizes needs, so that a sequence of queued surgeries finds it large enough
int reserve_surgery_scratch(msm_ctx *ctx, int nOld, int nNew, int Told, int Tnew);
// out (device, D x V(new)) = the weights applied to d_data (device, D x V(in)): barycentric_data_interpolation R/resampler.cpp:40-52
int apply_weights_dev(msm_ctx *ctx, const AdaptiveDev &w, const double *d_data, int D, double *d_out);
// the row offsets of device rows on the host (synchronises) and their last one, the number of entries
int fetch_row_ptr(msm_ctx *ctx, const AdaptiveDev &w, std::vector<int32_t> &row_ptr, size_t &nnz);
// the weights as host CSR; with an exclusion mask (or meshes of two contexts) the searches run on the GPU and the surgery on the host
int adaptive_weights(msm_mesh *in_mesh, msm_mesh *new_mesh, const double *excl, std::vector<int32_t> &row_ptr, std::vector<int32_t> &col,
                     std::vector<double> &val);
// the resampled mask, R/resampler.cpp:54-67: excl_out[k] = the row's weights applied to the mask itself, in entry order (nNew = row_ptr.size() - 1 values)
void resampled_mask(const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &col, const std::vector<double> &val, const double *excl, double *excl_out);

}  // namespace msm
