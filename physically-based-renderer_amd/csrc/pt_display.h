// pt_display.h — the display transform: metered exposure, tone-mapping operators, transfer functions.
//
// The renderer's images are scene-referred radiance in physical units; this file defines how one becomes a displayable RGBA8 (or an exposed RGBA16F for a viewer's
// own tonemapper).  It is compiled for host and device: the kernels (pt_display.hip) and the host evaluations (ptc_debug_display_pixel, ptc_debug_meter) call the
// same functions, and tests/display_reference.py restates them in numpy.  IEEE binary32, no contraction (-ffp-contract=off), in the order written; pt_fma
// = one rounding.  pt_pow, fmin2 / fmax2 and the ACES fit (aces_fit) are pt_device.h's host + device functions, the ones k_tonemap calls.
//
// Metering is exact in integers — no logarithm, no floating-point sum — so the device's result does not depend on the order it adds in:
//   luminance  l = (0.2126 r + 0.7152 g) + 0.0722 b                                   (pt_adaptive's unfused order)
//   class      alpha > 0 and l finite and > 0: metered; alpha > 0 and any other l (0, negative, NaN, inf): rejected; otherwise (alpha 0, negative or NaN): not counted
//   key        bits(l) >> 19: the biased exponent and the top four mantissa bits, 16 bins per stop, 4096 bins; denormals fall in keys 0..15; no clamp
//   trim       N metered pixels; lo_q = (uint32)(percentile_lo * 65536.0f), hi_q alike; n_lo = (N lo_q) >> 16, n_hi = (N hi_q) >> 16 in uint64; the samples whose
//              rank in ascending key order lies in [n_lo, n_hi) are kept, all of them if n_hi <= n_lo
//   mean       S = sum kept_k (2 k + 1), M = sum kept_k, Q = floor((S << 18) / M): the mean of the kept bins' centres' bit patterns — the piecewise-linear log2;
//              the metered luminance is uint_as_float((uint32)Q)
//   adaptation the state A is a uint32 in the same domain, 0 = none.  rate_q = (uint32)(adapt_rate * 65536.0f); A == 0 or rate_q == 65536: A = Q; otherwise
//              A = A + floor(((int64)Q - (int64)A) rate_q / 65536); M == 0 leaves A alone
//   scale      La = fmin2(fmax2(uint_as_float(A), min_luminance), max_luminance); E = gain (key / La) with auto_exposure on and A != 0, else E = gain
//
// Display, per pixel: c = rgb * E, then the operator, then per colour channel v = oetf(fmax2(v, 0)), clamp to [0, 1], (uint32)(int)(v * 255 + 0.5); alpha takes the
// clamp and the quantisation only, as in k_tonemap.  PTC_TONEMAP_ACES is k_tonemap's arithmetic: with E = 1 the bytes are ptc_tonemap_rgba8's.
//
// Non-finite input.  fmax2(NaN, 0) = 0 and pt_pow(x, y) = 0 unless x > 0, so every byte is definite:
//   a NaN channel      CLAMP: that channel 0.  ACES: the matrices mix it into all three: rgb 0.  REINHARD: lum is NaN, l = 0, s = 1: that channel 0, the others
//                      as without it.  PBR_NEUTRAL: min / max are fmin2 / fmax2 in the order written (fmin2(NaN, b) = b, fmin2(a, NaN) = NaN), so the result follows
//                      the channel's position; a NaN that reaches a channel gives 0.
//   +inf               CLAMP: 255.  ACES: rrt_odt(inf) = inf / inf = NaN: rgb 0 (what k_tonemap gives).  REINHARD: l = inf, s = inf / inf = NaN: rgb 0.
//                      PBR_NEUTRAL: peak = inf, np = 1, np / peak = 0, inf * 0 = NaN: the inf channel 0; the finite ones end at np g + c (1 - g) = 1: 255.
//   -inf               CLAMP, REINHARD (lum = -inf, l = 0, s = 1): that channel 0.  ACES: rgb 0.  PBR_NEUTRAL: the offset is -inf, that channel NaN and the others
//                      +inf, which the compression turns NaN: rgb 0.
//   alpha              NaN or negative 0, +inf 255.
// RGBA16F: half(rgb * E), alpha copied, round to nearest even, overflow to inf, half denormals kept (k_to_half's conversion); a NaN becomes 0x7e00.
#pragma once
#include "../../include/ptc.h"
#include "pt_device.h"

#define PT_DISPLAY_BINS 4096u
#define PT_DISPLAY_MAX_PIXELS (1u << 28)     // counts are uint32; S << 18 stays below 2^64

// what k_meter_reduce leaves in HBM, and what the display kernels read their exposure from
struct pt_display_state {
  uint32_t A;          // adaptation state, 0 = none
  uint32_t Q;          // the last metering's mean (0 when M was 0)
  uint32_t N, M;       // metered pixels, pixels kept by the trim
  uint32_t rejected;
  uint32_t pad[3];
};
static_assert(sizeof(pt_display_state) == 32, "pt_display_state is 32 bytes");

PT_HD uint32_t pt_display_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
PT_HD float pt_display_float(uint32_t u) { return __builtin_bit_cast(float, u); }
PT_HD float pt_display_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- metering -------------------------------------------------------------------------------------------------------------------------------------
// 0: not counted, 1: metered (key set), 2: rejected
PT_HD int pt_meter_classify(float r, float g, float b, float a, uint32_t& key) {
  if (!(a > 0.0f)) return 0;
  const float l = pt_display_lum(r, g, b);
  const uint32_t u = pt_display_bits(l);
  if (!(l > 0.0f) || u >= 0x7f800000u) return 2;
  key = u >> 19;
  return 1;
}
PT_HD void pt_meter_bounds(uint32_t N, float percentile_lo, float percentile_hi, uint64_t& n_lo, uint64_t& n_hi) {
  const uint32_t lo_q = (uint32_t)(percentile_lo * 65536.0f), hi_q = (uint32_t)(percentile_hi * 65536.0f);
  n_lo = ((uint64_t)N * lo_q) >> 16;
  n_hi = ((uint64_t)N * hi_q) >> 16;
  if (n_hi <= n_lo) { n_lo = 0; n_hi = N; }
}
// of a bin with `count` samples whose first has rank `before`: the samples with a rank in [n_lo, n_hi)
PT_HD uint64_t pt_meter_kept(uint64_t before, uint64_t count, uint64_t n_lo, uint64_t n_hi) {
  const uint64_t a = before > n_lo ? before : n_lo, b = before + count < n_hi ? before + count : n_hi;
  return b > a ? b - a : 0;
}
PT_HD uint32_t pt_meter_mean(uint64_t S, uint64_t M) { return M ? (uint32_t)((S << 18) / M) : 0u; }
PT_HD uint32_t pt_meter_adapt(uint32_t A, uint32_t Q, uint64_t M, float adapt_rate) {
  if (M == 0) return A;
  const uint32_t rate_q = (uint32_t)(adapt_rate * 65536.0f);
  if (A == 0u || rate_q == 65536u) return Q;
  const int64_t d = ((int64_t)Q - (int64_t)A) * (int64_t)rate_q;
  const int64_t step = d >= 0 ? d / 65536 : -((-d + 65535) / 65536);     // floor
  return (uint32_t)((int64_t)A + step);
}
PT_HD float pt_display_scale(const ptc_display_params& p, uint32_t A) {
  if (!p.auto_exposure || A == 0u) return p.gain;
  const float La = fmin2(fmax2(pt_display_float(A), p.min_luminance), p.max_luminance);
  return p.gain * (p.key / La);
}

// ---- operators ------------------------------------------------------------------------------------------------------------------------------------
template <int OP> PT_HD void pt_display_operator(float& r, float& g, float& b, float white) {
  if (OP == PTC_TONEMAP_ACES) {     // k_tonemap's
    const v3 o = aces_fit(V3(r, g, b));
    r = o.x; g = o.y; b = o.z;
  } else if (OP == PTC_TONEMAP_PBR_NEUTRAL) {     // Khronos PBR Neutral: startCompression 0.8 - 0.04 = 0.76, desaturation 0.15
    const float x = fmin2(r, fmin2(g, b));
    const float off = x < 0.08f ? x - 6.25f * (x * x) : 0.04f;
    r = r - off; g = g - off; b = b - off;
    const float peak = fmax2(r, fmax2(g, b));
    if (peak >= 0.76f) {
      const float np = 1.0f - (0.24f * 0.24f) / ((peak + 0.24f) - 0.76f);
      const float k = np / peak;
      r = r * k; g = g * k; b = b * k;
      const float q = 1.0f - 1.0f / (0.15f * (peak - np) + 1.0f);
      const float iq = 1.0f - q, nq = np * q;
      r = r * iq + nq; g = g * iq + nq; b = b * iq + nq;
    }
  } else if (OP == PTC_TONEMAP_REINHARD) {     // extended Reinhard on luminance
    const float l = fmax2(pt_display_lum(r, g, b), 0.0f);
    const float s = (1.0f + l / (white * white)) / (1.0f + l);
    r = r * s; g = g * s; b = b * s;
  }
}
template <int OETF> PT_HD float pt_display_oetf(float v) {
  if (OETF == PTC_OETF_SRGB) return v <= 0.0031308f ? 12.92f * v : 1.055f * pt_pow(v, 1.0f / 2.4f) - 0.055f;
  return pt_pow(v, 1.0f / 2.2f);
}
PT_HD uint32_t pt_display_unorm8(float v) {
  v = fmin2(fmax2(v, 0.0f), 1.0f);
  return (uint32_t)(int)(v * 255.0f + 0.5f);
}
template <int OP, int OETF> PT_HD uint32_t pt_display_pixel8(float r, float g, float b, float a, float E, float white) {
  r = r * E; g = g * E; b = b * E;
  pt_display_operator<OP>(r, g, b, white);
  return pt_display_unorm8(pt_display_oetf<OETF>(fmax2(r, 0.0f))) | (pt_display_unorm8(pt_display_oetf<OETF>(fmax2(g, 0.0f))) << 8) |
         (pt_display_unorm8(pt_display_oetf<OETF>(fmax2(b, 0.0f))) << 16) | (pt_display_unorm8(a) << 24);
}
PT_HD uint32_t pt_display_half_bits(float v) {
  if (v != v) return 0x7e00u;
  return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v);
}
PT_HD void pt_display_pixel16(float r, float g, float b, float a, float E, uint32_t& lo, uint32_t& hi) {
  lo = pt_display_half_bits(r * E) | (pt_display_half_bits(g * E) << 16);
  hi = pt_display_half_bits(b * E) | (pt_display_half_bits(a) << 16);
}

// ---- host: parameters -----------------------------------------------------------------------------------------------------------------------------
inline void pt_display_defaults(ptc_display_params& p) {
  p.gain = 1.0f; p.auto_exposure = 0; p.key = 0.18f; p.percentile_lo = 0.1f; p.percentile_hi = 0.9f; p.adapt_rate = 1.0f;
  p.min_luminance = 1e-4f; p.max_luminance = 1e6f; p.tonemap = PTC_TONEMAP_ACES; p.white = 4.0f; p.oetf = PTC_OETF_GAMMA22;
}
// nullptr when ptc_set_display would accept p
inline const char* pt_display_params_error(const ptc_display_params& p) {
  auto fin = [](float v) { return v - v == 0.0f; };
  if (!(fin(p.gain) && p.gain > 0.0f)) return "gain is not finite and > 0";
  if (p.auto_exposure != 0 && p.auto_exposure != 1) return "auto_exposure is not 0 or 1";
  if (!(fin(p.key) && p.key > 0.0f)) return "key is not finite and > 0";
  if (!(p.percentile_lo >= 0.0f && p.percentile_lo < 1.0f && p.percentile_hi > 0.0f && p.percentile_hi <= 1.0f && p.percentile_lo < p.percentile_hi))
    return "percentiles out of order (0 <= percentile_lo < percentile_hi <= 1)";
  if (!(p.adapt_rate >= 0.0f && p.adapt_rate <= 1.0f)) return "adapt_rate outside [0, 1]";
  if (!(fin(p.min_luminance) && p.min_luminance > 0.0f && fin(p.max_luminance) && p.max_luminance >= p.min_luminance)) return "luminance clamp (0 < min_luminance <= max_luminance, finite)";
  if (p.tonemap < PTC_TONEMAP_ACES || p.tonemap > PTC_TONEMAP_CLAMP) return "unknown tone-mapping operator";
  if (!(fin(p.white) && p.white > 0.0f)) return "white is not finite and > 0";
  if (p.oetf != PTC_OETF_GAMMA22 && p.oetf != PTC_OETF_SRGB) return "unknown transfer function";
  return nullptr;
}
// the host evaluation of one pixel with the operator and transfer function of p
inline uint32_t pt_display_host_pixel8(const ptc_display_params& p, float E, const float c[4]) {
#define PT_DISPLAY_CASE(OP)                                                                                                     \
  case OP: return p.oetf == PTC_OETF_SRGB ? pt_display_pixel8<OP, PTC_OETF_SRGB>(c[0], c[1], c[2], c[3], E, p.white)           \
                                          : pt_display_pixel8<OP, PTC_OETF_GAMMA22>(c[0], c[1], c[2], c[3], E, p.white);
  switch (p.tonemap) {
    PT_DISPLAY_CASE(PTC_TONEMAP_ACES)
    PT_DISPLAY_CASE(PTC_TONEMAP_PBR_NEUTRAL)
    PT_DISPLAY_CASE(PTC_TONEMAP_REINHARD)
    PT_DISPLAY_CASE(PTC_TONEMAP_CLAMP)
    default: break;
  }
#undef PT_DISPLAY_CASE
  return 0u;
}

// ---- the kernels (pt_display.hip); everything is queued on the stream given ------------------------------------------------------------------------
// hist: PT_DISPLAY_BINS counts followed by the rejected count (PT_DISPLAY_BINS + 1 words); the launcher zeroes them first
uint32_t pt_display_meter_grid_pixels();      // pixels one pass of k_meter_hist's grid covers
void pt_launch_meter(hipStream_t, const float4* image, uint32_t n_pixels, uint32_t* hist, pt_display_state* state, const ptc_display_params& p);
void pt_launch_display_rgba8(hipStream_t, const float4* image, uint32_t n_pixels, const pt_display_state* state, const ptc_display_params& p, uint32_t* out);
void pt_launch_display_half(hipStream_t, const float4* image, uint32_t n_pixels, const pt_display_state* state, const ptc_display_params& p, uint2* out);
