// ray_table.hpp -- what the direction table's build (ray_table.cpp) shares with its testing hooks (ray_table_check.cpp) and with the
// code that decides when a table is built (api.cpp).  build_ray_table and ray_certs_enabled are declared in internal.hpp.
#pragma once

#include "internal.hpp"

namespace msm {

constexpr double kRayShell = 1e-4;  // the table vouches for query points within this of radius kRad

// The leaves whose closed box meets [lo, hi] but which do not list triangle t (at most `cap` are collected; returns
// false when there are more)
bool lacking_leaves(const FlatOctree &o, int n, const double lo[3], const double hi[3], int t, int cap, std::vector<int> &lack);
// The box of the shell region above a triangle: every point of the shell whose direction lies in the spherical triangle of v[0..2] is
// within the sagitta of the flat triangle scaled to that radius, so the box of the unit vertices times the shell's two radii, grown by
// the sagitta, holds the region.  false (lo, hi unset): a vertex at the origin, or a triangle wider than 60 degrees.
bool ray_shell_box(const V3 v[3], double lo[3], double hi[3]);

// MSMHIP_DISABLE_RAYTABLE=1 (testing): no table is built, the complete search everywhere.  Read per call.
bool ray_table_disabled();
// MSMHIP_RAYTABLE: when the table of a cost target is built -- in the background (the default), on first use (sync), never (off).  Read per call.
enum class RayTableMode { background, sync, off };
RayTableMode ray_table_mode();

}  // namespace msm
