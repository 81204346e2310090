"""The two path numberings of csrc/pt_device.h (pt_path_id, pt_path_entry) on the host, no GPU needed.

A stand-alone program includes the header the kernels include and shows, for every batch shape of the list, that each numbering maps (entry, sample) onto
[0, n S) one to one, that pt_path_entry is its inverse, and that the ids are the stated expressions (s n + j; j S + s).  It is built as its own executable
with AddressSanitizer and UndefinedBehaviorSanitizer on the host code and run as such; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-renderer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include "pt_device.h"
#include <cstdio>
#include <vector>

static int check(int order, uint32_t n, uint32_t S) {
  const uint32_t total = n * S;
  std::vector<unsigned char> seen(total, 0);
  for (uint32_t j = 0; j < n; ++j)
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t p = pt_path_id(order, j, s, n, S);
      const uint32_t stated = order == PT_ORDER_PIXEL ? j * S + s : s * n + j;
      if (p != stated) { std::printf("order %d n %u S %u: id of (%u, %u) is %u, stated %u\n", order, n, S, j, s, p, stated); return 1; }
      if (p >= total) { std::printf("order %d n %u S %u: id %u of (%u, %u) outside [0, %u)\n", order, n, S, p, j, s, total); return 1; }
      if (seen[p]) { std::printf("order %d n %u S %u: id %u taken twice\n", order, n, S, p); return 1; }
      seen[p] = 1;
      uint32_t j2 = ~0u, s2 = ~0u;
      pt_path_entry(order, p, n, S, j2, s2);
      if (j2 != j || s2 != s) { std::printf("order %d n %u S %u: id %u inverts to (%u, %u), not (%u, %u)\n", order, n, S, p, j2, s2, j, s); return 1; }
    }
  for (uint32_t p = 0; p < total; ++p) {
    if (!seen[p]) { std::printf("order %d n %u S %u: id %u never formed\n", order, n, S, p); return 1; }
    uint32_t j = ~0u, s = ~0u;
    pt_path_entry(order, p, n, S, j, s);
    if (j >= n || s >= S || pt_path_id(order, j, s, n, S) != p) { std::printf("order %d n %u S %u: entry of id %u is (%u, %u)\n", order, n, S, p, j, s); return 1; }
  }
  return 0;
}

int main() {
  const uint32_t ns[] = {1, 63, 64, 851}, Ss[] = {1, 5, 64, 67, 453};
  int shapes = 0;
  for (int order : {(int)PT_ORDER_SAMPLE, (int)PT_ORDER_PIXEL})
    for (uint32_t n : ns)
      for (uint32_t S : Ss) {
        if (check(order, n, S)) return 1;
        ++shapes;
      }
  // a wave of bounce 0 under pixel-major: 64 consecutive ids are 64 samples of one entry when S is a multiple of 64
  for (uint32_t p = 0; p < 64u * 851u; ++p) {
    uint32_t j, s, j0, s0;
    pt_path_entry(PT_ORDER_PIXEL, p, 851u, 64u, j, s);
    pt_path_entry(PT_ORDER_PIXEL, p & ~63u, 851u, 64u, j0, s0);
    if (j != j0 || s != (p & 63u)) { std::printf("pixel-major wave of id %u is not one entry\n", p); return 1; }
  }
  std::printf("ok %d shapes\n", shapes);
  return 0;
}
"""


def test_both_numberings_are_bijections_with_the_stated_inverse(tmp_path):
    src, exe = tmp_path / "path_order_main.cpp", tmp_path / "path_order_main"
    src.write_text(PROGRAM)
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert r.stdout.strip() == "ok 40 shapes"
