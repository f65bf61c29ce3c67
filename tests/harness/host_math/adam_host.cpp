// TEST INFRASTRUCTURE (tests/test_adam_update_on_host.py): the PRODUCT's csrc/adam_update.h -- copied next to this file
// at test time, never edited -- compiled for the host; its "common.h" is the stand-in beside this file.
#include "adam_update.h"

// n elements of one tensor: g read, p, m and v updated in place
extern "C" void host_adam_update(const hgs_adam_tensor* T, const float* g, float* p, float* m, float* v, int64_t n) {
  for (int64_t i = 0; i < n; ++i) hgs::adam_update(*T, g[i], p[i], m[i], v[i]);
}
