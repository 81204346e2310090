// pt_temporal.hip — temporal accumulation: reproject the previous frame's accumulated image through the first-hit guides and blend the new frame in (gfx950).
//
// Specification: DESIGN.md §8c.  Per class-1 pixel with primitive `prim` and barycentrics (u, v):
//   1  X = (1-u-v) Pa' + u Pb' + v Pc', the positions of `prim` when the history was written (the snapshot, or the shading records when nothing moved since)
//   2  d = X - pos', z = d.f' (z <= 0: no history); x_prev = ((d.s' / z) / sx' + 1) 0.5 w - 0.5, y_prev likewise with u', sy', h
//   3  the four bilinear taps q around (x_prev, y_prev); valid iff inside, K'q = 1, n'q > 0 and |N'q . (X - P'q)| <= sigma_z Z'q pix'; W = sum of the valid
//      weights; W >= W_min: H, m1, m2, n = the weighted means over the valid taps, else all 0
//   4  D = C / max(A, 1e-3) (or C), L = lum(D); n_new = min(n + 1, max_history), a = 1 / n_new; D_new = (1-a) H + a D, m1 and m2 likewise from L and L L;
//      Var_t = max(m2_new - m1_new^2, 0); accumulated = D_new max(A, 1e-3) (or D_new) with the radiance's alpha
//   5  pixels of another class copy the radiance bit for bit and store n = 0
//   6  the new history: (D_new, n_new), (m1_new, m2_new, Var_t, a), bit copies of this frame's (N, Z) and (P, K)
// One pixel per thread, 32x8 tiles as k_dn_prepare lays them out: under camera motion the taps of a tile land in one neighbourhood of the history, so the
// second to fourth tap of a pixel come from L2.  Every load and store is 16 bytes but the primitive id and the barycentrics; a pixel reads 124 B of its own
// (radiance, three guides, id, barycentrics, three positions) plus up to 4 x 64 B of history and writes 96 B.  No atomics: a pixel has one owner, and the
// history set read is not the one written.
// Arithmetic: plain fp32 in the order of the specification, no contraction; the contract is the tolerance against a float64 evaluation
// (tests/test_gpu_temporal.py), and bit equality where the specification copies.
#include "pt_temporal.h"

#define TP_DEV __device__ __forceinline__
#define TP_BW 32
#define TP_BH 8
#define TP_EPS_A 1e-3f

namespace {
TP_DEV float tp_lum(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }
TP_DEV float tp_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__global__ __launch_bounds__(TP_BW * TP_BH) void k_tp_accumulate(TemporalArgs a) {
  const int x = (int)blockIdx.x * TP_BW + (int)(threadIdx.x % TP_BW), y = (int)blockIdx.y * TP_BH + (int)(threadIdx.x / TP_BW);
  if (x >= a.w || y >= a.h) return;
  const size_t p = (size_t)y * (size_t)a.w + (size_t)x;
  const float4 c = a.radiance[p], ak = a.g.albedo_class[p], nz = a.g.normal_depth[p], pk = a.g.pos_class[p];
  a.next.nz[p] = nz; a.next.pk[p] = pk;
  if (ak.w != 1.0f) {                                   // misses and emitters pass through and carry no history
    a.accumulated[p] = c;
    a.next.dn[p] = make_float4(c.x, c.y, c.z, 0.0f);
    a.next.mom[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    a.motion[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  float hx = 0.0f, hy = 0.0f, hz = 0.0f, hn = 0.0f, h1 = 0.0f, h2 = 0.0f, W = 0.0f, xp = 0.0f, yp = 0.0f;
  if (a.have_history) {
    const int prim = a.g.prim[p];
    const float2 uv = a.g.uv[p];
    const float4* rec = a.pos + (size_t)prim * a.pos_stride;
    const float4 pa = rec[0], pb = rec[1], pc = rec[2];
    const float w0 = (1.0f - uv.x) - uv.y;
    const float X = (w0 * pa.x + uv.x * pb.x) + uv.y * pc.x, Y = (w0 * pa.y + uv.x * pb.y) + uv.y * pc.y, Z = (w0 * pa.z + uv.x * pb.z) + uv.y * pc.z;
    const DevCamera& cm = a.cam_prev;
    const float dx = X - cm.pos[0], dy = Y - cm.pos[1], dz = Z - cm.pos[2];
    const float z = tp_dot3(dx, dy, dz, cm.f[0], cm.f[1], cm.f[2]);
    if (z > 0.0f) {
      xp = (((tp_dot3(dx, dy, dz, cm.s[0], cm.s[1], cm.s[2]) / z) / cm.sx + 1.0f) * 0.5f) * (float)a.w - 0.5f;
      yp = (((tp_dot3(dx, dy, dz, cm.u[0], cm.u[1], cm.u[2]) / z) / cm.sy + 1.0f) * 0.5f) * (float)a.h - 0.5f;
      // a tap can lie inside the image only for -1 < x_prev < w and -1 < y_prev < h (false for a NaN too): the conversions below are then in range
      if (xp > -1.0f && xp < (float)a.w && yp > -1.0f && yp < (float)a.h) {
        const float fx = floorf(xp), fy = floorf(yp);
        const int x0 = (int)fx, y0 = (int)fy;
        const float tx = xp - fx, ty = yp - fy;
        float sx_ = 0.0f, sy_ = 0.0f, sz_ = 0.0f, sn = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i, qy = y0 + j;
            if (qx < 0 || qx >= a.w || qy < 0 || qy >= a.h) continue;
            const size_t q = (size_t)qy * (size_t)a.w + (size_t)qx;
            const float4 pkq = a.prev.pk[q];
            if (pkq.w != 1.0f) continue;
            const float4 dq = a.prev.dn[q];
            if (!(dq.w > 0.0f)) continue;
            const float4 nzq = a.prev.nz[q];
            const float dist = fabsf(tp_dot3(nzq.x, nzq.y, nzq.z, X - pkq.x, Y - pkq.y, Z - pkq.z));
            if (!(dist <= (a.sigma_z * nzq.w) * a.pix_prev)) continue;
            const float4 mq = a.prev.mom[q];
            const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            W += b;
            sx_ += b * dq.x; sy_ += b * dq.y; sz_ += b * dq.z; sn += b * dq.w;
            s1 += b * mq.x; s2 += b * mq.y;
          }
        }
        if (W >= PTC_TEMPORAL_W_MIN) { hx = sx_ / W; hy = sy_ / W; hz = sz_ / W; hn = sn / W; h1 = s1 / W; h2 = s2 / W; }
      }
    }
  }
  const float ax = a.demodulate ? fmaxf(ak.x, TP_EPS_A) : 1.0f, ay = a.demodulate ? fmaxf(ak.y, TP_EPS_A) : 1.0f, az = a.demodulate ? fmaxf(ak.z, TP_EPS_A) : 1.0f;
  const float dx_ = a.demodulate ? c.x / ax : c.x, dy_ = a.demodulate ? c.y / ay : c.y, dz_ = a.demodulate ? c.z / az : c.z;
  const float L = tp_lum(dx_, dy_, dz_);
  const float n_new = fminf(hn + 1.0f, a.max_history);
  const float al = 1.0f / n_new, om = 1.0f - al;
  const float nx = om * hx + al * dx_, ny = om * hy + al * dy_, nzz = om * hz + al * dz_;
  const float m1 = om * h1 + al * L, m2 = om * h2 + al * (L * L);
  const float var = fmaxf(m2 - m1 * m1, 0.0f);
  a.next.dn[p] = make_float4(nx, ny, nzz, n_new);
  a.next.mom[p] = make_float4(m1, m2, var, al);
  a.motion[p] = make_float4(xp, yp, W, hn);
  a.accumulated[p] = a.demodulate ? make_float4(nx * ax, ny * ay, nzz * az, c.w) : make_float4(nx, ny, nzz, c.w);
}

// a pure stream: 48 B in at stride shade_stride, 48 B out, one float4 per thread
__global__ __launch_bounds__(256) void k_tp_snapshot(const float4* __restrict__ shade, uint32_t shade_stride, uint32_t n_units, float4* __restrict__ snapshot) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_units; i += gridDim.x * 256u) {
    const uint32_t prim = i / 3u, k = i - prim * 3u;
    snapshot[i] = shade[(size_t)prim * shade_stride + k];
  }
}
}  // namespace

void pt_launch_temporal_accumulate(hipStream_t s, const TemporalArgs& a) {
  const dim3 grid((unsigned)((a.w + TP_BW - 1) / TP_BW), (unsigned)((a.h + TP_BH - 1) / TP_BH));
  hipLaunchKernelGGL(k_tp_accumulate, grid, dim3(TP_BW * TP_BH), 0, s, a);
}

void pt_launch_temporal_snapshot(hipStream_t s, const float4* shade, uint32_t shade_stride, uint32_t n_prims, float4* snapshot) {
  if (n_prims == 0) return;
  const uint32_t n_units = 3u * n_prims;      // < 2^32: a primitive id has 28 bits
  uint32_t blocks = (n_units + 255u) / 256u;
  if (blocks > 2048u) blocks = 2048u;
  hipLaunchKernelGGL(k_tp_snapshot, dim3(blocks), dim3(256), 0, s, shade, shade_stride, n_units, snapshot);
}
