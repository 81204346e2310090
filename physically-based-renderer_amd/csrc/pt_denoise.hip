// pt_denoise.hip — variance-guided edge-avoiding à-trous filter over the first-hit guide buffers (gfx950).
//
// Per pixel p: radiance C, guides A (albedo), N (normal), Z (depth), K (class: 0 miss, 1 surface, 2 emitter), P = camera + Z · pixel-centre direction.
// Only class-1 pixels are filtered; the others pass through bit for bit and never contribute to a class-1 pixel.
//   prepare     D = C / max(A, 1e-3) (or C), L = lum(D); Var = normal-weighted variance of L over the same-class taps of the 7x7 window
//   iteration i step s = 2^i; S = sqrt(3x3 binomial blur of Var); 25 taps q = p + s (dx, dy) of the same class, weight
//               B3[dx] B3[dy] · max(0, Np·Nq)^sigma_n · exp(-|Np·(Pq - Pp)| / (sigma_p Zp pix s |(dx, dy)|); without Zp under an orthographic camera, a.pix_flat) · exp(-|Lq - Lp| / (sigma_l S + 1e-6));
//               D' = sum w Dq / sum w, Var' = sum w^2 Varq / (sum w)^2
//   the last iteration writes D' · max(A, 1e-3) with the radiance's alpha (re-modulation fused)
// Colour and variance travel as one float4, so a tap is three 16-byte loads: (D, Var), (N, Z), (P, K) — 48 B read + 16 B written per pixel and iteration when
// every tap after the first comes from a cache.  Steps 1 and 2 stage a 32x8 tile plus halo in LDS; larger steps gather rows from L2 / the Infinity Cache
// (at 1080p all four buffers, 4 x 33 MB, fit its 256 MiB).
// Arithmetic: plain fp32 in the order of the specification (taps row by row, no contraction), powf / expf of the device library: the contract is the
// tolerance against a float64 evaluation (tests/test_gpu_denoise.py), not bit equality.
#include "pt_denoise.h"

#define DN_DEV __device__ __forceinline__
#define DN_BW 32
#define DN_BH 8
#define DN_EPS_A 1e-3f
#define DN_EPS_L 1e-6f

namespace {
DN_DEV float dn_lum(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }
DN_DEV float dn_dot(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DN_DEV float4 dn_demodulate(float4 c, float4 ak, int demodulate) {
  if (!demodulate) return c;
  return make_float4(c.x / fmaxf(ak.x, DN_EPS_A), c.y / fmaxf(ak.y, DN_EPS_A), c.z / fmaxf(ak.z, DN_EPS_A), c.w);
}

// ---- prepare -------------------------------------------------------------------------------------------------------------------------------------------
#define DN_PREP_HALO 3
#define DN_PREP_TW (DN_BW + 2 * DN_PREP_HALO)
#define DN_PREP_TH (DN_BH + 2 * DN_PREP_HALO)
// colour: the filter's input, demodulated here when a.demodulate is set (the radiance), or a (D.rgb, n) image that is demodulated already (a.demodulate = 0:
// the temporal accumulation's).  TVAR: tvar holds (-, -, Var_t, a) per pixel, and where n >= 4 the variance is a Var_t, the variance of the accumulated mean,
// instead of the 7x7 estimate.
template <bool TVAR>
__global__ __launch_bounds__(DN_BW * DN_BH) void k_dn_prepare(DenoiseArgs a, const float4* __restrict__ colour, const float4* __restrict__ tvar, float4* cv_out) {
  __shared__ float4 s_nl[DN_PREP_TW * DN_PREP_TH];   // (N.xyz, L)
  __shared__ float s_k[DN_PREP_TW * DN_PREP_TH];     // class, -1 outside the image
  const int tx0 = (int)blockIdx.x * DN_BW - DN_PREP_HALO, ty0 = (int)blockIdx.y * DN_BH - DN_PREP_HALO;
  for (int i = (int)threadIdx.x; i < DN_PREP_TW * DN_PREP_TH; i += DN_BW * DN_BH) {
    const int gx = tx0 + i % DN_PREP_TW, gy = ty0 + i / DN_PREP_TW;
    float4 nl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float k = -1.0f;
    if (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) {
      const size_t g = (size_t)gy * (size_t)a.w + (size_t)gx;
      const float4 ak = a.g.albedo_class[g], nz = a.g.normal_depth[g];
      const float4 d = dn_demodulate(colour[g], ak, a.demodulate);
      nl = make_float4(nz.x, nz.y, nz.z, dn_lum(d.x, d.y, d.z));
      k = ak.w;
    }
    s_nl[i] = nl; s_k[i] = k;
  }
  __syncthreads();
  const int lx = (int)(threadIdx.x % DN_BW), ly = (int)(threadIdx.x / DN_BW);
  const int x = (int)blockIdx.x * DN_BW + lx, y = (int)blockIdx.y * DN_BH + ly;
  if (x >= a.w || y >= a.h) return;
  const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
  const float4 akp = a.g.albedo_class[p];
  const float4 d = dn_demodulate(colour[p], akp, a.demodulate);
  float var = 0.0f;
  if (TVAR && akp.w == 1.0f && d.w >= 4.0f) {
    const float4 t = tvar[p];
    var = t.w * t.z;
  } else if (akp.w == 1.0f) {
    const float4 np = s_nl[(ly + DN_PREP_HALO) * DN_PREP_TW + lx + DN_PREP_HALO];
    float m1 = 0.0f, m2 = 0.0f, cnt = 0.0f;
    for (int dy = 0; dy < 2 * DN_PREP_HALO + 1; ++dy) {
#pragma unroll
      for (int dx = 0; dx < 2 * DN_PREP_HALO + 1; ++dx) {
        const int i = (ly + dy) * DN_PREP_TW + lx + dx;
        if (s_k[i] != 1.0f) continue;          // outside the image, or another class
        const float4 nq = s_nl[i];
        const float g = powf(fmaxf(dn_dot(np, nq), 0.0f), a.sigma_n);
        const float gq = g * nq.w;
        m1 += gq; m2 += gq * nq.w; cnt += g;
      }
    }
    const float mean = m1 / cnt;
    var = fmaxf(m2 / cnt - mean * mean, 0.0f);
  }
  cv_out[p] = make_float4(d.x, d.y, d.z, var);
}

// ---- à-trous iteration -----------------------------------------------------------------------------------------------------------------------------------
// S > 0: step S, the tile (DN_BW + 4 S) x (DN_BH + 4 S) of all three buffers staged in LDS; S = 0: any step, taps gathered from global memory.
template <int S, bool LAST>
__global__ __launch_bounds__(DN_BW * DN_BH) void k_dn_atrous(DenoiseArgs a, int step_rt, const float4* __restrict__ cv_in, float4* __restrict__ out) {
  constexpr int HALO = 2 * S, TW = DN_BW + 2 * HALO, TH = DN_BH + 2 * HALO, TN = S > 0 ? TW * TH : 1;
  __shared__ float4 s_cv[TN], s_nz[TN], s_pk[TN];
  const int step = S > 0 ? S : step_rt;
  const int tx0 = (int)blockIdx.x * DN_BW - HALO, ty0 = (int)blockIdx.y * DN_BH - HALO;
  if (S > 0) {
    for (int i = (int)threadIdx.x; i < TN; i += DN_BW * DN_BH) {
      const int gx = tx0 + i % TW, gy = ty0 + i / TW;
      float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nz = cv, pk = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
      if (gx >= 0 && gx < a.w && gy >= 0 && gy < a.h) {
        const size_t g = (size_t)gy * (size_t)a.w + (size_t)gx;
        cv = cv_in[g]; nz = a.g.normal_depth[g]; pk = a.g.pos_class[g];
      }
      s_cv[i] = cv; s_nz[i] = nz; s_pk[i] = pk;
    }
    __syncthreads();
  }
  const int x = (int)blockIdx.x * DN_BW + (int)(threadIdx.x % DN_BW), y = (int)blockIdx.y * DN_BH + (int)(threadIdx.x / DN_BW);
  if (x >= a.w || y >= a.h) return;
  const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
  // the caller has checked that (qx, qy) lies inside the image (and, for S > 0, it then lies inside the tile: |offset| <= 2 S)
  auto load_cv = [&](int qx, int qy) { return S > 0 ? s_cv[(qy - ty0) * TW + (qx - tx0)] : cv_in[(size_t)qy * (size_t)a.w + (size_t)qx]; };
  auto load_nz = [&](int qx, int qy) { return S > 0 ? s_nz[(qy - ty0) * TW + (qx - tx0)] : a.g.normal_depth[(size_t)qy * (size_t)a.w + (size_t)qx]; };
  auto load_pk = [&](int qx, int qy) { return S > 0 ? s_pk[(qy - ty0) * TW + (qx - tx0)] : a.g.pos_class[(size_t)qy * (size_t)a.w + (size_t)qx]; };
  const float4 cvp = load_cv(x, y), pkp = load_pk(x, y);
  if (pkp.w != 1.0f) {                       // misses and emitters pass through
    out[p] = LAST ? a.radiance[p] : cvp;
    return;
  }
  const float4 nzp = load_nz(x, y);
  // S_p: the 3x3 (1/4, 1/2, 1/4)^2 blur of Var over the taps inside the image, renormalised
  float gv = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= a.w || qy < 0 || qy >= a.h) continue;
      const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
      gv += k * load_cv(qx, qy).w; gw += k;
    }
  }
  const float sd = sqrtf(fmaxf(gv / gw, 0.0f));
  const float lp = dn_lum(cvp.x, cvp.y, cvp.z);
  const float den_l = a.sigma_l * sd + DN_EPS_L;
  const float den_p = a.pix_flat ? a.sigma_p * a.pix : a.sigma_p * nzp.w * a.pix;
  float ax = 0.0f, ay = 0.0f, az = 0.0f, vacc = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + dx * step, qy = y + dy * step;
      if (qx < 0 || qx >= a.w || qy < 0 || qy >= a.h) continue;
      const float4 pkq = load_pk(qx, qy);
      if (pkq.w != 1.0f) continue;
      const float4 cvq = load_cv(qx, qy), nzq = load_nz(qx, qy);
      const float b3y = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f, b3x = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
      float w = (b3y * b3x) * powf(fmaxf(dn_dot(nzp, nzq), 0.0f), a.sigma_n);
      if (dx != 0 || dy != 0) {
        const int r2 = dx * dx + dy * dy;     // |(dx, dy)| as the nearest double, times the step, rounded once to fp32
        const double hyp = r2 == 1 ? 1.0 : r2 == 2 ? 1.4142135623730951 : r2 == 4 ? 2.0 : r2 == 5 ? 2.23606797749979 : 2.8284271247461903;
        const float sh = (float)((double)step * hyp);
        const float dist = fabsf((nzp.x * (pkq.x - pkp.x) + nzp.y * (pkq.y - pkp.y)) + nzp.z * (pkq.z - pkp.z));
        const float den = den_p * sh;
        w = w * expf(-dist / (den > 0.0f ? den : 1.0f));
      }
      w = w * expf(-fabsf(dn_lum(cvq.x, cvq.y, cvq.z) - lp) / den_l);
      ax += w * cvq.x; ay += w * cvq.y; az += w * cvq.z;
      vacc += (w * w) * cvq.w; wsum += w;
    }
  }
  float4 o = make_float4(ax / wsum, ay / wsum, az / wsum, vacc / (wsum * wsum));
  if (LAST) {
    if (a.demodulate) {
      const float4 ak = a.g.albedo_class[p];
      o.x = o.x * fmaxf(ak.x, DN_EPS_A); o.y = o.y * fmaxf(ak.y, DN_EPS_A); o.z = o.z * fmaxf(ak.z, DN_EPS_A);
    }
    o.w = a.radiance[p].w;
  }
  out[p] = o;
}

template <int S> void launch_atrous(hipStream_t s, const DenoiseArgs& a, int step, const float4* cv_in, float4* out, bool last) {
  const dim3 grid((unsigned)((a.w + DN_BW - 1) / DN_BW), (unsigned)((a.h + DN_BH - 1) / DN_BH));
  if (last) hipLaunchKernelGGL((k_dn_atrous<S, true>), grid, dim3(DN_BW * DN_BH), 0, s, a, step, cv_in, out);
  else hipLaunchKernelGGL((k_dn_atrous<S, false>), grid, dim3(DN_BW * DN_BH), 0, s, a, step, cv_in, out);
}
}  // namespace

void pt_launch_denoise_prepare(hipStream_t s, const DenoiseArgs& a, const float4* colour, const float4* tvar, float4* cv_out) {
  const dim3 grid((unsigned)((a.w + DN_BW - 1) / DN_BW), (unsigned)((a.h + DN_BH - 1) / DN_BH));
  if (tvar) hipLaunchKernelGGL(k_dn_prepare<true>, grid, dim3(DN_BW * DN_BH), 0, s, a, colour, tvar, cv_out);
  else hipLaunchKernelGGL(k_dn_prepare<false>, grid, dim3(DN_BW * DN_BH), 0, s, a, colour, tvar, cv_out);
}
void pt_launch_denoise_iteration(hipStream_t s, const DenoiseArgs& a, int iteration, const float4* cv_in, float4* out, bool last) {
  const int step = 1 << iteration;
  if (step == 1) launch_atrous<1>(s, a, step, cv_in, out, last);
  else if (step == 2) launch_atrous<2>(s, a, step, cv_in, out, last);
  else launch_atrous<0>(s, a, step, cv_in, out, last);
}
