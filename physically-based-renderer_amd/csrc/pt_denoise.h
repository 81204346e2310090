// pt_denoise.h — launchers of the variance-guided à-trous denoiser (pt_denoise.hip).  The filter is specified in DESIGN.md §"Denoiser"; its inputs are the
// radiance buffer and the first-hit guide buffers k_guides writes (ptc_internal.h: GuideBufs).
#pragma once
#include "ptc_internal.h"

struct DenoiseArgs {
  int w, h;
  float sigma_l, sigma_n, sigma_p;
  int demodulate;
  float pix;                    // 2 tan(fov_y / 2) / h: the world size of a pixel at unit distance
  int pix_flat;                 // 1: pix is the world size of a pixel at every depth (an orthographic camera, pt_camera.h): the plane-distance weight leaves Z out
  const float4* radiance;       // (C.rgb, alpha)
  GuideBufs g;
};
#define PTC_DENOISE_MAX_ITERATIONS 8
// colour, guides -> (D.rgb, Var): the demodulated colour and the variance of its luminance over the 7x7 window.  colour is the radiance (demodulated here when
// a.demodulate is set) or a (D.rgb, n) image demodulated already (a.demodulate = 0); tvar, when not NULL, holds (-, -, Var_t, a) per pixel: where n >= 4 the
// variance is a Var_t (pt_temporal.hip) instead of the window's estimate
void pt_launch_denoise_prepare(hipStream_t, const DenoiseArgs&, const float4* colour, const float4* tvar, float4* cv_out);
// iteration i (step 2^i): (D, Var) -> (D', Var'); the last one re-modulates and writes (colour, alpha of the radiance) instead
void pt_launch_denoise_iteration(hipStream_t, const DenoiseArgs&, int iteration, const float4* cv_in, float4* out, bool last);
