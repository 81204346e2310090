// pt_camera.hip — ray generation under the orthographic and the equirectangular projection (see pt_camera.h; the definition of every value is pt_proj_ray
// there, which the host evaluation calls too).
//
//   k_raygen_proj          one thread per path, k_raygen's path id -> (owned pixel j, sample first + s) mapping in the frame's path order (pt_device.h:
//                          pt_path_entry), so adaptive frames (the active-pixel list in DevFrame::owned), tile shares, sample ranges and both path orders need
//                          nothing of their own here.  One 4-byte load of the pixel index, four coalesced 16-byte stores: store_primary_ray
//                          (pt_pass_common.h).
//   k_raygen_guides_proj   the pixel-centre rays of a chunk of the frame, k_raygen_guides' record.
//   k_guides_pos_proj      rewrites the one field k_guides derived from a perspective ray: pos_class.xyz = o + Z d (a product and a sum per component, as k_guides
//                          writes it) with the projection's own origin and direction; Z and the class are read back from what k_guides wrote.
// Streaming kernels like k_raygen: 64 B written per path, every byte once.  Beside k_raygen's work EQUIRECT evaluates two sincos polynomials and a normalisation.
#include "pt_camera.h"
#include "pt_pass_common.h"

namespace {
__global__ __launch_bounds__(256) void k_raygen_proj(DevCamera cam, PtCamProj proj, DevFrame fr, DevQueues q, uint32_t first_sample, uint32_t n_samples) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= fr.n_owned * n_samples) return;
  uint32_t j, sl;
  pt_path_entry(fr.path_order, p, fr.n_owned, n_samples, j, sl);
  const uint32_t pixel = fr.owned[j];
  float o[3], d[3];
  uint32_t key;
  pt_proj_ray(cam, proj, fr.w, fr.h, fr.seed_hash, pixel, first_sample + sl, o, d, key);
  store_primary_ray(q, p, V3(o), V3(d), key, true);
}

__global__ __launch_bounds__(256) void k_raygen_guides_proj(DevCamera cam, PtCamProj proj, int w, int h, uint32_t first_pixel, uint32_t n, DevQueues q) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  float o[3], d[3];
  pt_proj_guide_ray(cam, proj, w, h, first_pixel + p, o, d);
  store_primary_ray(q, p, V3(o), V3(d), 0u, false);      // no key (its bits are 0.0f), and lpath is not a guide pass's
}

__global__ __launch_bounds__(256) void k_guides_pos_proj(DevCamera cam, PtCamProj proj, int w, int h, uint32_t first_pixel, uint32_t n,
                                                         const float4* __restrict__ normal_depth, float4* __restrict__ pos_class) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t pixel = first_pixel + j;
  float o[3], d[3];
  pt_proj_guide_ray(cam, proj, w, h, pixel, o, d);
  const float Z = normal_depth[pixel].w, K = pos_class[pixel].w;
  pos_class[pixel] = make_float4(o[0] + Z * d[0], o[1] + Z * d[1], o[2] + Z * d[2], K);
}
}  // namespace

void pt_launch_raygen_proj(hipStream_t s, const DevCamera& cam, const PtCamProj& proj, const DevFrame& fr, const DevQueues& q, uint32_t first_sample,
                           uint32_t n_samples) {
  const uint32_t n_paths = fr.n_owned * n_samples;
  if (!n_paths) return;
  hipLaunchKernelGGL(k_raygen_proj, dim3((n_paths + 255u) / 256u), dim3(256), 0, s, cam, proj, fr, q, first_sample, n_samples);
}

void pt_launch_raygen_guides_proj(hipStream_t s, const DevCamera& cam, const PtCamProj& proj, int w, int h, uint32_t first_pixel, uint32_t n, const DevQueues& q) {
  if (!n) return;
  hipLaunchKernelGGL(k_raygen_guides_proj, dim3((n + 255u) / 256u), dim3(256), 0, s, cam, proj, w, h, first_pixel, n, q);
}

void pt_launch_guides_pos_proj(hipStream_t s, const DevCamera& cam, const PtCamProj& proj, int w, int h, uint32_t first_pixel, uint32_t n,
                               const float4* normal_depth, float4* pos_class) {
  if (!n) return;
  hipLaunchKernelGGL(k_guides_pos_proj, dim3((n + 255u) / 256u), dim3(256), 0, s, cam, proj, w, h, first_pixel, n, normal_depth, pos_class);
}
