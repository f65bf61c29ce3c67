// TEST INFRASTRUCTURE (tests/test_hier_refit_rule_on_host.py): the PRODUCT's csrc/hier_refit_rule.h -- copied next to
// this file at test time, never edited -- compiled for the host; its "common.h" is the stand-in beside this file.
#include "hier_refit_rule.h"

// leaf boxes of n rows by mode (1 cube, 2 ellipsoid): lo, hi [n,3], extent [n], ok [n]
extern "C" void host_refit_leaves(const float* xyz, const float* log_scales, const float* rots, int64_t n, int32_t mode,
                                  float* lo, float* hi, float* extent, int32_t* ok) {
  for (int64_t i = 0; i < n; ++i) {
    const double x[3] = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
    const double ls[3] = {log_scales[i * 3], log_scales[i * 3 + 1], log_scales[i * 3 + 2]};
    const double q[4] = {rots[i * 4], rots[i * 4 + 1], rots[i * 4 + 2], rots[i * 4 + 3]};
    if (mode == hgs::kRefitCube) hgs::refit_leaf_cube(x, ls, lo + i * 3, hi + i * 3);
    else hgs::refit_leaf_ellipsoid(x, ls, q, lo + i * 3, hi + i * 3);
    extent[i] = hgs::refit_extent(lo + i * 3, hi + i * 3);
    ok[i] = hgs::refit_box_ok(lo + i * 3, hi + i * 3) ? 1 : 0;
  }
}

// the union of n boxes (lo, hi [n,3]) -> lo_out, hi_out [3]
extern "C" void host_refit_union(const float* lo, const float* hi, int64_t n, float* lo_out, float* hi_out) {
  for (int a = 0; a < 3; ++a) { lo_out[a] = lo[a]; hi_out[a] = hi[a]; }
  for (int64_t i = 1; i < n; ++i) hgs::refit_union(lo_out, hi_out, lo + i * 3, hi + i * 3);
}
