// TEST INFRASTRUCTURE (tests/test_hier_nodes_on_host.py): the PRODUCT's csrc/hier_nodes.h -- copied next to this file at
// test time, never edited -- compiled for the host; its "common.h" is the stand-in beside this file.
#include "hier_nodes.h"

// verdict[i] = node_layout's bits for node i; first_bad[0..3) = the first node with bit c set, through the library's own
// conversion of the unsigned minima
extern "C" void host_node_layout(const int32_t* nodes, int32_t N, uint32_t* verdict, int32_t* first_bad) {
  uint32_t minima[3] = {hgs::kNone, hgs::kNone, hgs::kNone};
  for (int64_t i = 0; i < N; ++i) {
    const uint32_t v = hgs::node_layout(nodes, i, N);
    verdict[i] = v;
    for (int c = 0; c < 3; ++c)
      if (((v >> c) & 1u) && (uint32_t)i < minima[c]) minima[c] = (uint32_t)i;
  }
  hgs::first_bad_from_minima(minima, 3, first_bad);
}

extern "C" int host_node_ints() { return hgs::kNodeInts; }
