// seg_layout_host.cpp — prints ptc_seg_layout and ptc_seg_slots (csrc/ptc_internal.h) for "n max_seg" pairs read from stdin, one line "n max_seg n_seg seg_len slots"
// each: tests/test_pass_policies_host.py holds its Python restatement (tests/pass_policies.py) to this table.
#include "ptc_internal.h"
#include <cstdio>
int main() {
  unsigned n, max_seg;
  while (std::scanf("%u %u", &n, &max_seg) == 2) {
    uint32_t n_seg = 0, seg_len = 0;
    ptc_seg_layout(n, max_seg, n_seg, seg_len);
    std::printf("%u %u %u %u %zu\n", n, max_seg, n_seg, seg_len, ptc_seg_slots(n, max_seg));
  }
  return 0;
}
