// pt_adaptive.hip — adaptive sampling on gfx950: moments, error estimate, keep rule + stable compaction of the active list, per-pixel resolve.
//
// A frame in adaptive mode keeps, per owned pixel, the RGB sum (accum, as always), m1 = sum l_k, m2 = sum l_k l_k of the per-sample luminance
// l_k = (0.2126 r + 0.7152 g) + 0.0722 b, and the number of samples received.  The path kernels see the frame as DevFrame{n_active, active pixels}; the kernels
// here map an active entry j back to its owned position slot[j].
//   k_ad_accumulate     pure stream: 16 B per sample and entry in, 28 B of state read and written per entry; <true>: + the six sums of products of the
//                       channels (rr, gg, bb, rg | rb, gb), a float4 and a float2 per entry: 52 B of state (ptc_set_sample_covariance)
//   k_ad_error          mean = m1 / n, var = max(m2 / n - mean mean, 0), e = sqrt(var / n) / (mean + 0.01), flag = e > threshold: one byte per active pixel
//   k_ad_compact_*      keep = some flagged pixel within Chebyshev distance `radius`, inside the image and the pixel's own 32x32 tile; then a STABLE compaction
//                       of (pixel, slot): per-block counts, one block scans them (as k_scan does), ballot + mbcnt prefix per wave and an LDS prefix over the
//                       block's waves place every kept entry — no atomics, so the list keeps the tile-Morton order and is the same on every run
//   k_ad_resolve        accum / (float)count per owned pixel
//   k_ad_sampled_*      the denoiser's input from the sums (§8d): the biased covariance of the samples' channels, the variance of the (demodulated) luminance
//                       as its quadratic form, and the demodulated radiance with the count — the two images pt_launch_denoise_prepare takes
// Arithmetic: IEEE binary32 in the order written (the Makefile's -ffp-contract=off and correctly rounded division and square root): tests/adaptive_reference.py
// performs the same operations in numpy and the sample counts are compared exactly.
#include "pt_adaptive.h"
#include "pt_device.h"

#define AD_SCAN_BLOCK 1024

namespace {
__device__ __forceinline__ float ad_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_init(uint32_t n_owned, const uint32_t* __restrict__ owned, uint32_t* __restrict__ pix, uint32_t* __restrict__ slot) {
  const uint32_t j = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  if (j >= n_owned) return;
  pix[j] = owned[j]; slot[j] = j;
}

// one sample's additions to an entry's sums, in the order every form of k_ad_accumulate performs them
template <bool COV>
__device__ __forceinline__ void ad_add(const float4 L, float4& a, float2& m, float4& q4, float2& q2) {
  a.x = a.x + L.x; a.y = a.y + L.y; a.z = a.z + L.z;
  const float l = ad_lum(L.x, L.y, L.z);
  m.x = m.x + l; m.y = m.y + l * l;
  if (COV) {
    q4.x = q4.x + L.x * L.x; q4.y = q4.y + L.y * L.y; q4.z = q4.z + L.z * L.z; q4.w = q4.w + L.x * L.y;
    q2.x = q2.x + L.x * L.z; q2.y = q2.y + L.y * L.z;
  }
}

// PIXEL_MAJOR: the batch numbers its paths entry by entry (PT_ORDER_PIXEL); a wave then owns PT_ACC_ROWS entries (AD_PM_ENTRIES a block) and takes their rows of
// lpath through LDS a 1-KiB run per row at a time, as k_accumulate_pixel_major does (pt_device.h, pt_lpath_tile_*); the sums and their order are the same.
// The loop bounds are the block's.
#define AD_PM_ENTRIES (PTC_AD_BLOCK / 64u * PT_ACC_ROWS)
template <bool COV, bool PIXEL_MAJOR>
__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_accumulate(uint32_t n_active, const uint32_t* __restrict__ slot, const float4* __restrict__ lpath, float4* __restrict__ accum,
                                                                float2* __restrict__ moments, uint32_t* __restrict__ count, float4* __restrict__ cov4, float2* __restrict__ cov2,
                                                                uint32_t n_samples) {
  __shared__ float4 s_tile[PIXEL_MAJOR ? PTC_AD_BLOCK / 64 : 1][PIXEL_MAJOR ? PT_ACC_TILE_UNITS : 1];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t j0 = PIXEL_MAJOR ? blockIdx.x * AD_PM_ENTRIES + wv * PT_ACC_ROWS : blockIdx.x * PTC_AD_BLOCK + wv * 64u, j = j0 + lane;
  const bool live = j < n_active && (!PIXEL_MAJOR || lane < PT_ACC_ROWS);      // this lane owns entry j
  if (!PIXEL_MAJOR && !live) return;
  const uint32_t o = live ? slot[j] : 0u;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float2 m = make_float2(0.0f, 0.0f);
  float4 q4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float2 q2 = make_float2(0.0f, 0.0f);
  if (live) { a = accum[o]; m = moments[o]; }
  if (COV && live) { q4 = cov4[o]; q2 = cov2[o]; }
  if (PIXEL_MAJOR) {
    float4* tile = s_tile[wv];
    const uint32_t first = pt_path_id(PT_ORDER_PIXEL, j, 0u, n_active, n_samples), n_tiles = pt_lpath_tiles(n_samples);
    PtAccRegs v = pt_lpath_tile_fetch(lpath, j0, n_active, n_samples, 0u, lane);
    for (uint32_t k = 0; k < n_tiles; ++k) {
      pt_lpath_tile_put(tile, lane, v);
      __syncthreads();
      if (k + 1u < n_tiles) v = pt_lpath_tile_fetch(lpath, j0, n_active, n_samples, k + 1u, lane);
      if (live)
        for (uint32_t t = 0; t < PT_ACC_RUN; ++t)
          if (pt_lpath_tile_has(first, n_samples, k, t)) ad_add<COV>(tile[lane * PT_ACC_ROW + t], a, m, q4, q2);
      __syncthreads();
    }
    if (!live) return;
  } else {
    for (uint32_t s = 0; s < n_samples; ++s) ad_add<COV>(lpath[pt_path_id(PT_ORDER_SAMPLE, j, s, n_active, n_samples)], a, m, q4, q2);
  }
  accum[o] = a; moments[o] = m; count[o] += n_samples;
  if (COV) { cov4[o] = q4; cov2[o] = q2; }
}

__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_error(uint32_t n_active, const uint32_t* __restrict__ pix, const uint32_t* __restrict__ slot, const float2* __restrict__ moments,
                                                           uint8_t* __restrict__ flags, float fn, float threshold) {
  const uint32_t j = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  if (j >= n_active) return;
  const float2 m = moments[slot[j]];
  const float mean = m.x / fn;
  const float var = fmaxf(m.y / fn - mean * mean, 0.0f);
  const float e = sqrtf(var / fn) / (mean + 0.01f);
  flags[pix[j]] = e > threshold ? 1 : 0;
}

// keep predicate per active entry + the number of kept entries per block
__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_compact_count(uint32_t n_active, const uint32_t* __restrict__ pix, const uint8_t* __restrict__ flags, uint8_t* __restrict__ keep,
                                                                   uint32_t* __restrict__ block_tot, int w, int h, int radius) {
  __shared__ uint32_t s_w[PTC_AD_BLOCK / 64];
  const uint32_t j = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  bool k = false;
  if (j < n_active) {
    const uint32_t p = pix[j];
    const int px = (int)(p % (uint32_t)w), py = (int)(p / (uint32_t)w);
    // the window, clipped to the image and to the pixel's tile
    const int tx0 = px / PTC_AD_TILE * PTC_AD_TILE, ty0 = py / PTC_AD_TILE * PTC_AD_TILE;
    const int x0 = max(px - radius, tx0), x1 = min(min(px + radius, tx0 + PTC_AD_TILE - 1), w - 1);
    const int y0 = max(py - radius, ty0), y1 = min(min(py + radius, ty0 + PTC_AD_TILE - 1), h - 1);
    for (int y = y0; y <= y1; ++y)
      for (int x = x0; x <= x1; ++x) k = k || flags[(size_t)y * (size_t)w + (size_t)x] != 0;
    keep[j] = k ? 1 : 0;
  }
  const unsigned long long b = __ballot(k);
  if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int i = 0; i < PTC_AD_BLOCK / 64; ++i) t += s_w[i];
    block_tot[blockIdx.x] = t;
  }
}

// one block: block_tot[0, n_blocks) -> its exclusive prefix in place, the total to n_out[0]
__global__ __launch_bounds__(AD_SCAN_BLOCK) void k_ad_compact_scan(uint32_t n_blocks, uint32_t* __restrict__ block_tot, uint32_t* __restrict__ n_out) {
  __shared__ uint32_t s_w[AD_SCAN_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_blocks; base += AD_SCAN_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_blocks ? block_tot[i] : 0u;
    uint32_t incl = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63u) s_w[wid] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < AD_SCAN_BLOCK / 64; ++k) { const uint32_t t = s_w[k]; if (k < wid) before += t; all += t; }
    if (i < n_blocks) block_tot[i] = carry + before + (incl - v);
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) n_out[0] = carry;
}

// kept entries to their places: block prefix + the waves before this one + the kept lanes before this one
__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_compact_write(uint32_t n_active, const uint32_t* __restrict__ pix, const uint32_t* __restrict__ slot, const uint8_t* __restrict__ keep,
                                                                   const uint32_t* __restrict__ block_pre, uint32_t* __restrict__ pix_out, uint32_t* __restrict__ slot_out) {
  __shared__ uint32_t s_w[PTC_AD_BLOCK / 64];
  const uint32_t j = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  const bool k = j < n_active && keep[j] != 0;
  const unsigned long long b = __ballot(k);
  const uint32_t in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
  const uint32_t wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) s_w[wid] = (uint32_t)__popcll(b);
  __syncthreads();
  if (!k) return;
  uint32_t dst = block_pre[blockIdx.x] + in_wave;
  for (uint32_t i = 0; i < wid; ++i) dst += s_w[i];
  if (dst >= n_active) return;   // cannot happen (a prefix of kept entries of a list of n_active): the output arrays hold n_active entries
  pix_out[dst] = pix[j]; slot_out[dst] = slot[j];
}

__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_resolve(uint32_t n_owned, const uint32_t* __restrict__ owned, const float4* __restrict__ accum, const uint32_t* __restrict__ count,
                                                             float4* __restrict__ radiance) {
  const uint32_t o = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  const uint32_t n = count[o];
  if (n == 0) return;
  const float4 a = accum[o];
  const float fn = (float)n;
  radiance[owned[o]] = make_float4(a.x / fn, a.y / fn, a.z / fn, 1.0f);
}

#define AD_EPS_A 1e-3f
__device__ __forceinline__ float4 ad_demodulate(float4 c, float4 ak, int demodulate) {
  if (!demodulate) return c;
  return make_float4(c.x / fmaxf(ak.x, AD_EPS_A), c.y / fmaxf(ak.y, AD_EPS_A), c.z / fmaxf(ak.z, AD_EPS_A), c.w);
}

// every pixel: (D, 0) and zeros, what a pixel the frame does not own keeps
__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_sampled_fill(uint32_t n_pixels, const float4* __restrict__ albedo, const float4* __restrict__ radiance, int demodulate,
                                                                  float4* __restrict__ colour, float4* __restrict__ svar) {
  const uint32_t p = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  if (p >= n_pixels) return;
  const float4 d = ad_demodulate(radiance[p], albedo[p], demodulate);
  colour[p] = make_float4(d.x, d.y, d.z, 0.0f);
  svar[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// one owned entry per thread; the owned list is in tile-Morton order, so a wave writes whole 32-pixel rows of a tile
__global__ __launch_bounds__(PTC_AD_BLOCK) void k_ad_sampled_variance(uint32_t n_owned, const uint32_t* __restrict__ owned, const float4* __restrict__ accum,
                                                                      const float4* __restrict__ cov4, const float2* __restrict__ cov2, const uint32_t* __restrict__ count,
                                                                      const float4* __restrict__ albedo, const float4* __restrict__ radiance, int demodulate,
                                                                      float4* __restrict__ colour, float4* __restrict__ svar, uint32_t n_pixels) {
  const uint32_t o = blockIdx.x * PTC_AD_BLOCK + threadIdx.x;
  if (o >= n_owned) return;
  const uint32_t p = owned[o];
  if (p >= n_pixels) return;      // cannot happen (the owned list holds pixels of the frame): both images hold n_pixels entries
  const uint32_t n = count[o];
  const float4 ak = albedo[p];
  const float4 d = ad_demodulate(radiance[p], ak, demodulate);
  if (n == 0) {
    colour[p] = make_float4(d.x, d.y, d.z, 0.0f);
    svar[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float4 s = accum[o], q4 = cov4[o];
  const float2 q2 = cov2[o];
  const float fn = (float)n;
  const float mr = s.x / fn, mg = s.y / fn, mb = s.z / fn;
  const float crr = q4.x / fn - mr * mr, cgg = q4.y / fn - mg * mg, cbb = q4.z / fn - mb * mb;
  const float crg = q4.w / fn - mr * mg, crb = q2.x / fn - mr * mb, cgb = q2.y / fn - mg * mb;
  float ar = 0.2126f, ag = 0.7152f, ab = 0.0722f;
  if (demodulate) { ar = ar / fmaxf(ak.x, AD_EPS_A); ag = ag / fmaxf(ak.y, AD_EPS_A); ab = ab / fmaxf(ak.z, AD_EPS_A); }
  const float v = (((ar * ar) * crr + (ag * ag) * cgg) + (ab * ab) * cbb) + 2.0f * ((((ar * ag) * crg + (ar * ab) * crb)) + (ag * ab) * cgb);
  colour[p] = make_float4(d.x, d.y, d.z, fn);
  svar[p] = make_float4(0.0f, 0.0f, fmaxf(v, 0.0f), 1.0f / fn);
}
}  // namespace

void pt_launch_ad_init(hipStream_t s, uint32_t n_owned, const uint32_t* owned, uint32_t* pix, uint32_t* slot) {
  if (!n_owned) return;
  hipLaunchKernelGGL(k_ad_init, dim3(pt_ad_blocks(n_owned)), dim3(PTC_AD_BLOCK), 0, s, n_owned, owned, pix, slot);
}
template <bool PIXEL_MAJOR>
static void launch_ad_accumulate(hipStream_t s, uint32_t n_active, const uint32_t* slot, const float4* lpath, float4* accum, const DevAdaptive& ad, uint32_t n_samples) {
  if (!n_active) return;
  const dim3 grid(PIXEL_MAJOR ? (n_active + AD_PM_ENTRIES - 1u) / AD_PM_ENTRIES : pt_ad_blocks(n_active));
  if (ad.cov4) hipLaunchKernelGGL((k_ad_accumulate<true, PIXEL_MAJOR>), grid, dim3(PTC_AD_BLOCK), 0, s, n_active, slot, lpath, accum, ad.moments, ad.count, ad.cov4, ad.cov2, n_samples);
  else hipLaunchKernelGGL((k_ad_accumulate<false, PIXEL_MAJOR>), grid, dim3(PTC_AD_BLOCK), 0, s, n_active, slot, lpath, accum, ad.moments, ad.count, ad.cov4, ad.cov2, n_samples);
}
void pt_launch_ad_accumulate(hipStream_t s, uint32_t n_active, const uint32_t* slot, const float4* lpath, float4* accum, const DevAdaptive& ad, uint32_t n_samples, int path_order) {
  if (path_order == PT_ORDER_PIXEL) launch_ad_accumulate<true>(s, n_active, slot, lpath, accum, ad, n_samples);
  else launch_ad_accumulate<false>(s, n_active, slot, lpath, accum, ad, n_samples);
}
void pt_launch_ad_error(hipStream_t s, uint32_t n_active, const uint32_t* pix, const uint32_t* slot, const DevAdaptive& ad, uint32_t n, float threshold) {
  if (!n_active) return;
  hipLaunchKernelGGL(k_ad_error, dim3(pt_ad_blocks(n_active)), dim3(PTC_AD_BLOCK), 0, s, n_active, pix, slot, (const float2*)ad.moments, ad.flags, (float)n, threshold);
}
void pt_launch_ad_compact(hipStream_t s, uint32_t n_active, const uint32_t* pix, const uint32_t* slot, uint32_t* pix_out, uint32_t* slot_out, const DevAdaptive& ad, int w, int h, int radius) {
  const uint32_t nb = pt_ad_blocks(n_active);
  if (nb) hipLaunchKernelGGL(k_ad_compact_count, dim3(nb), dim3(PTC_AD_BLOCK), 0, s, n_active, pix, (const uint8_t*)ad.flags, ad.keep, ad.block_tot, w, h, radius);
  hipLaunchKernelGGL(k_ad_compact_scan, dim3(1), dim3(AD_SCAN_BLOCK), 0, s, nb, ad.block_tot, ad.n_out);
  if (nb) hipLaunchKernelGGL(k_ad_compact_write, dim3(nb), dim3(PTC_AD_BLOCK), 0, s, n_active, pix, slot, (const uint8_t*)ad.keep, (const uint32_t*)ad.block_tot, pix_out, slot_out);
}
void pt_launch_ad_resolve(hipStream_t s, uint32_t n_owned, const uint32_t* owned, const float4* accum, const uint32_t* count, float4* radiance) {
  if (!n_owned) return;
  hipLaunchKernelGGL(k_ad_resolve, dim3(pt_ad_blocks(n_owned)), dim3(PTC_AD_BLOCK), 0, s, n_owned, owned, accum, count, radiance);
}
void pt_launch_ad_sampled_variance(hipStream_t s, uint32_t n_owned, const uint32_t* owned, const float4* accum, const DevAdaptive& ad, const float4* albedo, const float4* radiance,
                                   int demodulate, float4* colour, float4* svar, uint32_t n_pixels, bool fill_all) {
  if (fill_all && n_pixels) hipLaunchKernelGGL(k_ad_sampled_fill, dim3(pt_ad_blocks(n_pixels)), dim3(PTC_AD_BLOCK), 0, s, n_pixels, albedo, radiance, demodulate, colour, svar);
  if (!n_owned) return;
  hipLaunchKernelGGL(k_ad_sampled_variance, dim3(pt_ad_blocks(n_owned)), dim3(PTC_AD_BLOCK), 0, s, n_owned, owned, accum, (const float4*)ad.cov4, (const float2*)ad.cov2,
                     (const uint32_t*)ad.count, albedo, radiance, demodulate, colour, svar, n_pixels);
}
