// pt_temporal.h — launchers of the temporal accumulation (pt_temporal.hip).  The step is specified in DESIGN.md §8c; its inputs are the radiance buffer, the
// first-hit guide buffers of the current frame (ptc_internal.h: GuideBufs), the history of the previous frame and that frame's primitive positions.
#pragma once
#include "ptc_internal.h"

// One history set, full-frame arrays indexed by pixel.  Two sets ping-pong: a step reads one and writes the other.
struct TemporalSet {
  float4* dn;       // (D.rgb, n): the accumulated demodulated colour and the (fractional) number of frames in it; n = 0 on pixels that are not class 1
  float4* mom;      // (m1, m2, Var_t, a): first and second moment of the luminance, their variance, the blend factor of the step that wrote them
  float4* nz;       // bit copy of the frame's (N, Z)
  float4* pk;       // bit copy of the frame's (P, K)
};

struct TemporalArgs {
  int w, h;
  int have_history;             // 0: every pixel is a first frame, `prev` and `pos` are not read
  int demodulate;
  float max_history;            // 1..1024 as a float
  float sigma_z;
  float pix_prev;               // 2 sy' / h of the history's camera
  DevCamera cam_prev;           // the history's camera
  const float4* radiance;       // (C.rgb, alpha)
  GuideBufs g;                  // the current frame's guides
  const float4* pos;            // positions of the history's frame: (Pa, Pb, Pc) = pos[prim * pos_stride + 0..2].xyz
  uint32_t pos_stride;          // 3 (the snapshot) or the scene's shade_stride (the shading records themselves, when nothing moved since)
  TemporalSet prev, next;
  float4* accumulated;          // the accumulated image (re-modulated, alpha of the radiance)
  float4* motion;               // (x_prev, y_prev, W, n_reprojected)
};
#define PTC_TEMPORAL_MAX_HISTORY 1024
#define PTC_TEMPORAL_W_MIN 0.01f
// steps 1-6 of the specification for every pixel of the frame
void pt_launch_temporal_accumulate(hipStream_t, const TemporalArgs&);
// the first three float4 of every primitive's shading record -> snapshot[3 * prim + 0..2]
void pt_launch_temporal_snapshot(hipStream_t, const float4* shade, uint32_t shade_stride, uint32_t n_prims, float4* snapshot);
