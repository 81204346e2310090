// pt_adaptive.h — adaptive sampling: per-pixel sample moments, the error estimate and the active-pixel list (pt_adaptive.hip; DESIGN.md "Adaptive sampling").
#pragma once
#include "ptc_internal.h"

#define PTC_AD_TILE 32       // the neighbourhood of the keep rule is clipped to the pixel's ownership tile: kTile of ptc_scene.cpp
#define PTC_AD_BLOCK 256     // threads per block of every kernel here; one active entry per thread
#define PTC_AD_MAX_RADIUS 2

// The state of an adaptive frame on the device.  "Owned position" o = index into the frame's owned-pixel list (the order of accum); "active entry" j = index into
// the active list, which holds (pixel, owned position) pairs in the order of the owned list (tile-Morton) with the stopped pixels taken out.
struct DevAdaptive {
  float2* moments;        // [n_owned] (m1, m2) = sums of the per-sample luminance and of its square, in sample order
  uint32_t* count;        // [n_owned] samples received
  uint8_t* flags;         // [w * h] 1 where an ACTIVE pixel's error estimate exceeds the threshold; stopped and unowned pixels read 0
  uint8_t* keep;          // [n_active] scratch of the compaction: the keep predicate per active entry
  uint32_t* block_tot;    // [ceil(n_active / PTC_AD_BLOCK)] scratch: kept entries per block, then their exclusive prefix
  uint32_t* n_out;        // [1] length of the new active list
  float4* cov4;           // [n_owned] (rr, gg, bb, rg): sums of the products of the per-sample radiance's channels, in sample order; NULL in a frame that
  float2* cov2;           // [n_owned] (rb, gb)          does not keep the sample covariance (ptc_set_sample_covariance)
};
inline uint32_t pt_ad_blocks(uint32_t n) { return (n + PTC_AD_BLOCK - 1u) / PTC_AD_BLOCK; }

// active list := the owned list, slot[j] = j
void pt_launch_ad_init(hipStream_t, uint32_t n_owned, const uint32_t* owned, uint32_t* pix, uint32_t* slot);
// k_accumulate's three additions per sample on accum[slot[j]], then m1, m2 and count; sample s of active entry j is lpath[pt_path_id(path_order, j, s, n_active,
// n_samples)] (pt_device.h): s * n_active + j in a sample-major batch, j * n_samples + s in a pixel-major one, whose rows a wave transposes through LDS.  With
// ad.cov4 set the six product sums follow (further instantiations: a sample-major frame without them runs the kernel it always ran)
void pt_launch_ad_accumulate(hipStream_t, uint32_t n_active, const uint32_t* slot, const float4* lpath, float4* accum, const DevAdaptive&, uint32_t n_samples, int path_order);
// flags[pixel] = e > threshold for every active entry, n = the samples every active pixel has received
void pt_launch_ad_error(hipStream_t, uint32_t n_active, const uint32_t* pix, const uint32_t* slot, const DevAdaptive&, uint32_t n, float threshold);
// the keep rule (a flagged pixel within `radius`, inside the image and the tile) + the stable compaction of (pix, slot) into (pix_out, slot_out); the new length goes to ad.n_out
void pt_launch_ad_compact(hipStream_t, uint32_t n_active, const uint32_t* pix, const uint32_t* slot, uint32_t* pix_out, uint32_t* slot_out, const DevAdaptive&, int w, int h, int radius);
// radiance[owned[o]] = accum[o] / (float)count[o], alpha 1; a pixel without samples is left alone
void pt_launch_ad_resolve(hipStream_t, uint32_t n_owned, const uint32_t* owned, const float4* accum, const uint32_t* count, float4* radiance);
// The denoiser's input from the per-sample statistics, per owned entry o with pixel = owned[o] and n = count[o]:
//   colour[pixel] = (D.rgb, (float)n), D = radiance[pixel] / max(albedo, 1e-3) (or the radiance), svar[pixel] = (0, 0, Var_s, 1 / (float)n); n = 0: (D, 0) and zeros.
// fill_all: the frame does not own every pixel, so a pass over all w * h pixels writes (D, 0) and zeros first.
void pt_launch_ad_sampled_variance(hipStream_t, uint32_t n_owned, const uint32_t* owned, const float4* accum, const DevAdaptive&, const float4* albedo, const float4* radiance,
                                   int demodulate, float4* colour, float4* svar, uint32_t n_pixels, bool fill_all);
