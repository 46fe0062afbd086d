// smooth_device.hpp -- the expressions of smooth_data (R/resampler.cpp:168-230) that decide a neighbourhood and weigh its members, written once:
// k_smooth (kernels.hip) and the row builder of a smoothing plan (smooth_plan_kernels.hip) give the same bits because they share them
// (-ffp-contract=off: every product, sum and quotient below is rounded on its own).
#pragma once

#include "geom.hpp"

namespace msm {

// 1 / sqrt(2 pi sigma^2), :205
__device__ __forceinline__ double smooth_gain(double sigma) { return 1 / sqrt(2 * M_PI * sigma * sigma); }
// can a chunk of 64 unit vectors with bounding ball b (k_chunk_bounds) hold a member?  (a | ref) <= (centre | ref) + radius for every vector a of the
// chunk, so a chunk whose bound stays below cos(ang) holds none; a NaN anywhere keeps the chunk
__device__ __forceinline__ bool smooth_chunk_candidate(const double4 &b, const V3 &ref, double cosang) {
    return !(b.x * ref.x + b.y * ref.y + b.z * ref.z + b.w < cosang);
}
// (actual | ref) >= cos(ang), :190
__device__ __forceinline__ bool smooth_member(const V3 &a, const V3 &ref, double cosang) { return dot(a, ref) >= cosang; }
// |ref - a| of a member, :192
__device__ __forceinline__ double smooth_chord(const V3 &ref, const V3 &a) { return norm(sub(ref, a)); }
// gain * exp(-g^2 / (2 sigma^2)) with g the geodesic distance that belongs to the chord on the sphere of radius RAD, :193-206
__device__ __forceinline__ double smooth_weight(double chord, double gain, double sigma) {
    const double g = 2 * kRad * asin(chord / (2 * kRad));
    return gain * exp(-(g * g) / (2 * sigma * sigma));
}

}  // namespace msm
