// pt_lens.hip — ray generation through a thin lens (see pt_lens.h; the definition of every value is pt_lens_ray there, which the host evaluation calls too).
//
//   k_raygen_lens   one thread per path, k_raygen's path id -> (owned pixel j, sample first + s) mapping in the frame's path order (pt_device.h: pt_path_entry;
//                   sample-major j = p % n_owned, s = p / n_owned, pixel-major j = p / n_samples, s = p % n_samples), so adaptive frames (the
//                   active-pixel list in DevFrame::owned), tile shares and sample ranges need nothing of their own here.  One 4-byte load of the pixel index,
//                   four coalesced 16-byte stores: store_primary_ray (pt_pass_common.h).
// A streaming kernel like k_raygen: 64 B written per path, every byte once.  Beside k_raygen's work it hashes two more RNG dimensions and evaluates a square
// root and one (disk) or two (blades) sincos polynomials; profiles/lens_1080p.txt has the two kernels' times at equal path counts.
#include "pt_lens.h"
#include "pt_pass_common.h"

namespace {
__global__ __launch_bounds__(256) void k_raygen_lens(DevCamera cam, ptc_lens_params lens, DevFrame fr, DevQueues q, uint32_t first_sample, uint32_t n_samples) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= fr.n_owned * n_samples) return;
  uint32_t j, sl;
  pt_path_entry(fr.path_order, p, fr.n_owned, n_samples, j, sl);
  const uint32_t pixel = fr.owned[j];
  float o[3], d[3];
  uint32_t key;
  pt_lens_ray(cam, lens, fr.w, fr.h, fr.seed_hash, pixel, first_sample + sl, o, d, key);
  store_primary_ray(q, p, V3(o), V3(d), key, true);
}
}  // namespace

void pt_launch_raygen_lens(hipStream_t s, const DevCamera& cam, const ptc_lens_params& lens, const DevFrame& fr, const DevQueues& q, uint32_t first_sample,
                           uint32_t n_samples) {
  const uint32_t n_paths = fr.n_owned * n_samples;
  if (!n_paths) return;
  const dim3 grid((n_paths + 255u) / 256u);
  hipLaunchKernelGGL(k_raygen_lens, grid, dim3(256), 0, s, cam, lens, fr, q, first_sample, n_samples);
}
