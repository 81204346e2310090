// pt_deform.hip — morph targets and skinning of one mesh's object-space vertices on the device (see pt_deform.h; the definition of every value is
// pt_deform_eval_vertex in pt_deform.cpp, and both sides call the same pt_deform_morph / pt_deform_skin).
//
//   k_deform   one thread per vertex of the posed mesh: base vertex (three 16-byte loads), the deltas of every target (target-major: lane v reads
//              12 bytes at (k n + v) 12, so a wave reads 768 contiguous bytes per array and target), the 24-byte skin record (three 8-byte loads),
//              four joint matrices, and three 16-byte stores into the mesh's slice of the object-space vertex array.
// A streaming kernel: 48 B read + 48 B written + 24 B of skin + 36 B per target and vertex, every byte touched once; nothing to tile.
//
// The joint matrices (48 B per joint, a few kilobytes) are read by data-dependent index.  Two variants are compiled: kLds = false reads them from
// global memory (they stay in the vector L1 / L2 after the first wave), kLds = true copies up to kLdsJoints of them into LDS per block first.
// The default is the global-memory variant; PTC_DEFORM_LDS=1 in the environment selects the LDS one for meshes whose joints fit.  WHICH IS FASTER HAS
// NOT BEEN MEASURED: the default is provisional, chosen because it needs no barrier and no LDS, and tools/deform_bench.py run with and without the
// variable is the comparison that should settle it.  Both variants write the same bytes (tests/test_gpu_deform.py runs each).
#include "pt_deform.h"

#include <cstdlib>
#include <cstring>

namespace {
constexpr int kBlock = 256;
constexpr uint32_t kLdsJoints = 256;      // 12 KB of LDS

template <bool kLds>
__global__ __launch_bounds__(kBlock) void k_deform(const DevDeform d) {
  __shared__ float sJ[kLds ? kLdsJoints * 12 : 1];
  const float* J = d.pose + d.n_targets;
  if (kLds) {
    for (uint32_t i = threadIdx.x; i < d.n_joints * 12u; i += kBlock) sJ[i] = J[i];
    __syncthreads();
    J = sJ;
  }
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= d.n_verts) return;
  const float4* src = reinterpret_cast<const float4*>(d.base + v);      // a 48-byte record on a 16-byte boundary
  const float4 r0 = src[0], r1 = src[1], r2 = src[2];                   // (p.xyz, n.x) (n.yz, t.xy) (t.zw, uv)
  float p[3] = {r0.x, r0.y, r0.z}, n[3] = {r0.w, r1.x, r1.y}, t[3] = {r1.z, r1.w, r2.x};
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t k = 0; k < d.n_targets; ++k) {
    const size_t at = ((size_t)k * d.n_verts + v) * 3;
    const float w = d.pose[k];
    float dp[3] = {d.dp[at], d.dp[at + 1], d.dp[at + 2]}, dn[3] = {0.0f, 0.0f, 0.0f}, dt[3] = {0.0f, 0.0f, 0.0f};
    if (d.dn) { dn[0] = d.dn[at]; dn[1] = d.dn[at + 1]; dn[2] = d.dn[at + 2]; }
    if (d.dt) { dt[0] = d.dt[at]; dt[1] = d.dt[at + 1]; dt[2] = d.dt[at + 2]; }
    pt_deform_morph(p, n, t, w, dp, d.dn ? dn : zero, d.dt ? dt : zero);
  }
  if (d.skin) {
    const uint2* sr = reinterpret_cast<const uint2*>(d.skin + v);        // 24 bytes on an 8-byte boundary
    const uint2 s0 = sr[0], s1 = sr[1], s2 = sr[2];
    const uint32_t j0 = s0.x & 0xffffu, j1 = s0.x >> 16, j2 = s0.y & 0xffffu, j3 = s0.y >> 16;
    const float a[4] = {__uint_as_float(s1.x), __uint_as_float(s1.y), __uint_as_float(s2.x), __uint_as_float(s2.y)};
    pt_deform_skin(p, n, t, a, J + (size_t)j0 * 12, J + (size_t)j1 * 12, J + (size_t)j2 * 12, J + (size_t)j3 * 12);
  }
  float4* dst = reinterpret_cast<float4*>(d.out + v);
  dst[0] = make_float4(p[0], p[1], p[2], n[0]);
  dst[1] = make_float4(n[1], n[2], t[0], t[1]);
  dst[2] = make_float4(t[2], r2.y, r2.z, r2.w);                          // tangent.w and the texcoord are copied
}
}  // namespace

void pt_launch_deform(hipStream_t st, const DevDeform& d) {
  if (!d.n_verts) return;
  const uint32_t blocks = (d.n_verts + kBlock - 1) / kBlock;
  const char* e = std::getenv("PTC_DEFORM_LDS");
  const bool lds = e && std::strcmp(e, "1") == 0 && d.skin && d.n_joints <= kLdsJoints;
  if (lds) hipLaunchKernelGGL(k_deform<true>, dim3(blocks), dim3(kBlock), 0, st, d);
  else hipLaunchKernelGGL(k_deform<false>, dim3(blocks), dim3(kBlock), 0, st, d);
}
