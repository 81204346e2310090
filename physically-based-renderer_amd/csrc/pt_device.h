// pt_device.h — the arithmetic of the path-tracing core (gfx950), written once for host and device.
//
// Arithmetic contract (DESIGN.md §"Arithmetic contract"): IEEE binary32, correctly rounded
// + - * / sqrt (-fhip-fp32-correctly-rounded-divide-sqrt), NO implicit contraction
// (-ffp-contract=off): a fused multiply-add happens exactly where __builtin_fmaf is written.
// No libm / ocml transcendental on the render path: sin/cos/pow are the polynomials below.
// These rules make every value reproducible on any IEEE machine, which is what lets the parity
// tests demand (near) bit-equality instead of a statistical comparison.
//
// Two parts.  PT_HD (host + device): v3 and its operators, the scalar helpers, the RNG hash, the polynomials and the ACES
// fit — plain IEEE expressions that need no GPU.  The feature headers (pt_lens.h, pt_probes.h, pt_lights.h, pt_display.h)
// define their values through these, and the library's host evaluations (ptc_debug_*, ptc_frame_begin's seed hash) call the
// same functions the kernels call: a value has ONE expression in the product, and the host computes the bytes the device
// writes because it runs the same text under the same contract.  PT_DEV (device only): the BSDF, the ray / box / triangle
// code and the wave helpers, which only kernels use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pt_exact.h"

#define PT_DEV __device__ __forceinline__
#define PT_HD __host__ __device__ __forceinline__

#define PT_LEAF_MAX 2
#define PT_RR_START 3u
#define PT_RR_PMIN 0.05f
#define PT_ALPHA_MIN 0.001f
#define PT_T_INF 3.0e38f
#define PT_PI 3.14159265358979323846f
#define PT_INV_PI 0.31830988618379067154f
#define PT_HALF_PI 1.57079632679489661923f
#define PT_ZNEAR 0.01f   // CameraData.hpp:25
#define PT_ZFAR 1024.0f  // CameraData.hpp:26

struct v3 { float x, y, z; };

PT_HD v3 V3(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_HD v3 V3(const float a[3]) { return V3(a[0], a[1], a[2]); }
PT_HD v3 operator+(v3 a, v3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_HD v3 operator-(v3 a, v3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_HD v3 operator-(v3 a) { return V3(-a.x, -a.y, -a.z); }
PT_HD v3 operator*(v3 a, float s) { return V3(a.x * s, a.y * s, a.z * s); }
PT_HD float pt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_HD float dot3(v3 a, v3 b) { return pt_fma(a.z, b.z, pt_fma(a.y, b.y, a.x * b.x)); }
PT_HD v3 cross3(v3 a, v3 b) {
  return V3(pt_fma(a.y, b.z, -(a.z * b.y)), pt_fma(a.z, b.x, -(a.x * b.z)), pt_fma(a.x, b.y, -(a.y * b.x)));
}
// pt_sqrt, pt_rnorm: pt_exact.h.  inv = 1 / sqrt(dot) in two roundings, as ever; on the device ONE test of the squared length guards both (a squared length
// inside [2^-32, 2^32) has its root and the root's reciprocal inside [2^-16, 2^16]), anything else — a zero vector among them — takes the compiler's expansions
PT_HD v3 normalize3(v3 a) { float inv = pt_rnorm(dot3(a, a)); return a * inv; }
PT_HD v3 vfma(v3 a, float s, v3 b) { return V3(pt_fma(a.x, s, b.x), pt_fma(a.y, s, b.y), pt_fma(a.z, s, b.z)); }
PT_HD float fmin2(float a, float b) { return a < b ? a : b; }
PT_HD float fmax2(float a, float b) { return a > b ? a : b; }
PT_HD float max3c(v3 a) { return fmax2(fmax2(a.x, a.y), a.z); }
PT_HD float luminance(v3 c) { return pt_fma(c.z, 0.0722f, pt_fma(c.y, 0.7152f, c.x * 0.2126f)); }

// ---- RNG: counter-based hash keyed (seed, pixel, sample) then (bounce, dim) -------------------
PT_HD uint32_t pcg(uint32_t v) {
  uint32_t s = v * 747796405u + 2891336453u;
  uint32_t w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
  return (w >> 22) ^ w;
}
PT_HD uint32_t path_key(uint32_t seed_hash, uint32_t pixel, uint32_t sample) {
  return pcg(pixel + pcg(sample + seed_hash));
}
PT_HD uint32_t seed_hash(uint64_t seed) { return pcg((uint32_t)seed + pcg((uint32_t)(seed >> 32))); }   // what DevFrame.seed_hash holds
PT_HD float rng_f(uint32_t key, uint32_t bounce, uint32_t dim) {
  uint32_t x = pcg(pcg(bounce * 8u + dim) ^ key);
  return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// ---- path numbering of a batch: (entry j of the owned / active list, sample s of the batch) <-> path id p = queue slot at bounce 0 ----
// A batch of n entries x S samples numbers its paths in one of two orders (DevFrame::path_order):
//   sample-major  p = s n + j   a wave of bounce 0 carries one sample of 64 neighbouring entries
//   pixel-major   p = j S + s   a wave of bounce 0 carries 64 samples of one entry (S >= 64), and an entry's samples lie side by side in lpath
// n S fits 32 bits (ptc_frame_begin).  Every kernel and host evaluation that forms or inverts a path id calls these two.
enum { PT_ORDER_SAMPLE = 0, PT_ORDER_PIXEL = 1 };
PT_HD uint32_t pt_path_id(int order, uint32_t j, uint32_t s, uint32_t n, uint32_t S) { return order == PT_ORDER_PIXEL ? j * S + s : s * n + j; }
PT_HD void pt_path_entry(int order, uint32_t p, uint32_t n, uint32_t S, uint32_t& j, uint32_t& s) {
  if (order == PT_ORDER_PIXEL) { j = p / S; s = p % S; }
  else { j = p % n; s = p / n; }
}

// ---- sin(2πu), cos(2πu), u ∈ [0,1): quadrant + octant reduction, Taylor on [0, π/4] ------------
PT_HD void sincos2pi(float u, float& so, float& co) {
  float x4 = u * 4.0f;
  int q = (int)x4;
  if (q > 3) q = 3;
  float r = x4 - (float)q;
  bool swap = r > 0.5f;
  float rr = swap ? 1.0f - r : r;
  float x = rr * PT_HALF_PI;
  float x2 = x * x;
  float ps = pt_fma(x2, pt_fma(x2, pt_fma(x2, pt_fma(x2, 2.7557319e-6f, -1.9841270e-4f), 8.3333333e-3f), -1.6666667e-1f), 1.0f);
  float s = x * ps;
  float c = pt_fma(x2, pt_fma(x2, pt_fma(x2, pt_fma(x2, 2.4801587e-5f, -1.3888889e-3f), 4.1666667e-2f), -0.5f), 1.0f);
  if (swap) { float t = s; s = c; c = t; }
  float S, C;
  if (q == 0) { S = s; C = c; }
  else if (q == 1) { S = c; C = -s; }
  else if (q == 2) { S = -s; C = -c; }
  else { S = -c; C = s; }
  so = S; co = C;
}

// ---- x^y for x > 0 (else 0): exp2(y·log2 x) by polynomial --------------------------------------
PT_HD float pt_log2(float x) {
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  int e = (int)((u >> 23) & 0xffu) - 127;
  float m = __builtin_bit_cast(float, (u & 0x007fffffu) | 0x3f800000u);
  if (m > 1.41421356f) { m = m * 0.5f; e += 1; }
  float z = (m - 1.0f) / (m + 1.0f);
  float z2 = z * z;
  float p = pt_fma(z2, pt_fma(z2, pt_fma(z2, pt_fma(z2, 0.3205989f, 0.4121984f), 0.5770780f), 0.9617967f), 2.8853901f);
  return pt_fma(z, p, (float)e);
}
PT_HD float pt_exp2(float x) {
  if (x < -126.0f) return 0.0f;
  if (x > 127.0f) x = 127.0f;
  float fl = __builtin_floorf(x);
  float f = x - fl;
  float p = pt_fma(f, pt_fma(f, pt_fma(f, pt_fma(f, pt_fma(f, 1.8775767e-3f, 8.9893397e-3f), 5.5826318e-2f), 2.4015361e-1f), 6.9315308e-1f), 9.9999994e-1f);
  return p * __builtin_bit_cast(float, (uint32_t)((int)fl + 127) << 23);
}
PT_HD float pt_pow(float x, float y) {
  if (!(x > 0.0f)) return 0.0f;
  return pt_exp2(y * pt_log2(x));
}

// ---- atan2(y, x) in (-pi, pi]: octant reduction + odd minimax polynomial on [0,1] (max error ~1e-5 rad) --------
PT_HD float pt_atan2(float y, float x) {
  const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  const float mx = fmax2(ax, ay), mn = fmin2(ax, ay);
  if (!(mx > 0.0f)) return 0.0f;
  const float a = mn / mx, a2 = a * a;
  const float p = pt_fma(a2, pt_fma(a2, pt_fma(a2, pt_fma(a2, pt_fma(a2, -0.01172120f, 0.05265332f), -0.11643287f), 0.19354346f), -0.33262347f), 0.99997726f);
  float r = a * p;
  if (ay > ax) r = PT_HALF_PI - r;
  if (x < 0.0f) r = PT_PI - r;
  if (y < 0.0f) r = -r;
  return r;
}

// ---- R9 tonemap: ACES fit (matrices as GLSL reads them: column-major, i.e. transposed — SURVEY §3.4) ------------
PT_HD float rrt_odt(float c) {
  const float num = c * (c + 0.0245786f) - 0.000090537f;
  const float den = c * (0.983729f * c + 0.4329510f) + 0.238081f;
  return num / den;
}
PT_HD v3 aces_input(v3 c) {
  return V3(0.59719f * c.x + 0.07600f * c.y + 0.02840f * c.z, 0.35458f * c.x + 0.90834f * c.y + 0.13383f * c.z, 0.04823f * c.x + 0.01566f * c.y + 0.83777f * c.z);
}
PT_HD v3 aces_output(v3 f) {
  return V3(1.60475f * f.x + -0.10208f * f.y + -0.00327f * f.z, -0.53108f * f.x + 1.10813f * f.y + -0.07276f * f.z, -0.07367f * f.x + -0.00605f * f.y + 1.07602f * f.z);
}
PT_HD v3 aces_fit(v3 c) { const v3 i = aces_input(c); return aces_output(V3(rrt_odt(i.x), rrt_odt(i.y), rrt_odt(i.z))); }

// ==== device only =================================================================================
// ---- P6: BSDF in the local frame of the shading normal (z = n) ---------------------------------
struct bsdf_t { v3 cd, f0; float alpha; int ggx; };

PT_DEV bsdf_t make_bsdf(v3 base, float metallic, float roughness, bool lambert_class) {
  bsdf_t b;
  float mt = metallic;
  b.ggx = !lambert_class;
  b.cd = base * (1.0f - mt);
  float d = 0.04f * (1.0f - mt);
  b.f0 = V3(pt_fma(base.x, mt, d), pt_fma(base.y, mt, d), pt_fma(base.z, mt, d));
  float a = roughness * roughness;
  b.alpha = fmax2(a, PT_ALPHA_MIN);
  return b;
}
PT_DEV float smith_g1(float x, float a2) { return (2.0f * x) / (x + pt_sqrt(pt_fma(1.0f - a2, x * x, a2))); }
PT_DEV v3 schlick(v3 f0, float voh) {
  float m = 1.0f - voh; if (m < 0.0f) m = 0.0f;
  float m2 = m * m; float m5 = m2 * m2 * m;
  return V3(pt_fma(1.0f - f0.x, m5, f0.x), pt_fma(1.0f - f0.y, m5, f0.y), pt_fma(1.0f - f0.z, m5, f0.z));
}
PT_DEV float spec_prob(const bsdf_t& b, float nov) {
  if (!b.ggx) return 0.0f;
  float ld = luminance(b.cd);
  if (!(ld > 0.0f)) return 1.0f;
  float lf = luminance(schlick(b.f0, nov));
  float p = lf / (lf + ld);
  return fmin2(fmax2(p, 0.1f), 0.9f);
}
PT_DEV void bsdf_eval(const bsdf_t& b, v3 wo, v3 wi, float ps, v3& f, float& pdf) {
  float nol = wi.z;
  v3 fd = b.cd * PT_INV_PI;
  float pd = nol * PT_INV_PI;
  if (!b.ggx) { f = fd; pdf = pd; return; }
  float nov = fmax2(wo.z, 1e-4f);
  v3 h = normalize3(wo + wi);
  float noh = h.z, voh = dot3(wo, h);
  float a2 = b.alpha * b.alpha;
  float dd = pt_fma(noh * noh, a2 - 1.0f, 1.0f);
  float D = a2 / (PT_PI * dd * dd);
  float gv = smith_g1(nov, a2), gl = smith_g1(nol, a2);
  v3 F = schlick(b.f0, voh);
  float sp = (D * gv * gl) / (4.0f * nov * nol);
  f = V3(pt_fma(F.x, sp, fd.x), pt_fma(F.y, sp, fd.y), pt_fma(F.z, sp, fd.z));
  float pspec = (gv * D) / (4.0f * nov);
  pdf = pt_fma(ps, pspec, (1.0f - ps) * pd);
}
PT_DEV bool bsdf_sample(const bsdf_t& b, v3 wo, float ps, float ul, float s1, float s2, v3& wi) {
  float sn, cs; sincos2pi(s2, sn, cs);
  float r = pt_sqrt(s1);
  if (ul < ps) {  // GGX VNDF (Heitz 2018)
    float a = b.alpha;
    v3 vh = normalize3(V3(a * wo.x, a * wo.y, wo.z));
    float lensq = pt_fma(vh.y, vh.y, vh.x * vh.x);
    v3 t1 = V3(1.0f, 0.0f, 0.0f);
    if (lensq > 0.0f) { float il = pt_rnorm(lensq); t1 = V3(-vh.y * il, vh.x * il, 0.0f); }
    v3 t2 = cross3(vh, t1);
    float p1 = r * cs, p2 = r * sn;
    float s = 0.5f * (1.0f + vh.z);
    p2 = pt_fma(1.0f - s, pt_sqrt(fmax2(0.0f, 1.0f - p1 * p1)), s * p2);
    float pz = pt_sqrt(fmax2(0.0f, 1.0f - p1 * p1 - p2 * p2));
    v3 nh = vfma(t1, p1, vfma(t2, p2, vh * pz));
    v3 h = normalize3(V3(a * nh.x, a * nh.y, fmax2(0.0f, nh.z)));
    float voh = dot3(wo, h);
    wi = V3(pt_fma(2.0f * voh, h.x, -wo.x), pt_fma(2.0f * voh, h.y, -wo.y), pt_fma(2.0f * voh, h.z, -wo.z));
  } else {        // cosine hemisphere
    wi = V3(r * cs, r * sn, pt_sqrt(fmax2(0.0f, 1.0f - s1)));
  }
  return wi.z > 0.0f;
}
// branchless orthonormal basis (Duff et al. 2017)
PT_DEV void onb(v3 n, v3& t, v3& b) {
  float sg = __builtin_copysignf(1.0f, n.z);
  float a = -1.0f / (sg + n.z);
  float bb = n.x * n.y * a;
  t = V3(pt_fma(sg * n.x, n.x * a, 1.0f), sg * bb, -sg * n.x);
  b = V3(bb, pt_fma(n.y, n.y * a, sg), -n.y);
}

// ---- ray / box / triangle ----------------------------------------------------------------------
struct ray_t { v3 o, d, inv, ood; };
PT_DEV float safe_dir(float d) { return __builtin_fabsf(d) < 1e-20f ? __builtin_copysignf(1e-20f, d) : d; }
PT_DEV ray_t make_ray(v3 o, v3 d) {
  ray_t r; r.o = o; r.d = d;
  r.inv = V3(1.0f / safe_dir(d.x), 1.0f / safe_dir(d.y), 1.0f / safe_dir(d.z));
  r.ood = V3(o.x * r.inv.x, o.y * r.inv.y, o.z * r.inv.z);
  return r;
}
PT_DEV bool box_hit(const ray_t& r, float lx, float ly, float lz, float hx, float hy, float hz, float tmin, float tlimit, float& tn) {
  float x0 = pt_fma(lx, r.inv.x, -r.ood.x), x1 = pt_fma(hx, r.inv.x, -r.ood.x);
  float y0 = pt_fma(ly, r.inv.y, -r.ood.y), y1 = pt_fma(hy, r.inv.y, -r.ood.y);
  float z0 = pt_fma(lz, r.inv.z, -r.ood.z), z1 = pt_fma(hz, r.inv.z, -r.ood.z);
  float tnear = fmax2(fmax2(fmin2(x0, x1), fmin2(y0, y1)), fmax2(fmin2(z0, z1), tmin));
  float tfar = fmin2(fmin2(fmax2(x0, x1), fmax2(y0, y1)), fmin2(fmax2(z0, z1), tlimit));
  tn = tnear;
  return tnear <= tfar;
}
// Möller–Trumbore on (v0,e1,e2); CULL = R6 back-face culling (front = det > 0)
template <bool CULL>
PT_DEV bool tri_test(const ray_t& r, v3 v0, v3 e1, v3 e2, float& t, float& u, float& v) {
  v3 p = cross3(r.d, e2);
  float det = dot3(e1, p);
  if (CULL ? !(det > 0.0f) : (det == 0.0f)) return false;
  float inv = 1.0f / det;
  v3 tv = r.o - v0;
  float uu = dot3(tv, p) * inv;
  if (!(uu >= 0.0f && uu <= 1.0f)) return false;
  v3 q = cross3(tv, e1);
  float vv = dot3(r.d, q) * inv;
  if (!(vv >= 0.0f && uu + vv <= 1.0f)) return false;
  t = dot3(e2, q) * inv; u = uu; v = vv;
  return true;
}

// ---- wave64 helpers ------------------------------------------------------------------------------
PT_DEV uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
PT_DEV uint32_t mbcnt64(uint64_t m) {   // number of set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ---- a pixel-major batch's path radiance, transposed: what k_accumulate and k_ad_accumulate read under PT_ORDER_PIXEL -------------
// An entry's S samples are S x 16 contiguous bytes of lpath (its row), and the rows of consecutive entries lie back to back.  One lane per entry
// reading its own row would touch 64 lines per load, so a wave owns PT_ACC_ROWS entries [j0, j0 + PT_ACC_ROWS) and takes their rows through LDS a
// tile at a time: tile k holds, of every row, the k-th run of PT_ACC_RUN units (1 KiB) counted from the 128-byte line the row starts in, so that
// load i of a tile is ONE coalesced 1-KiB read of row i on line boundaries, lane = unit inside the run.  Lane r < PT_ACC_ROWS then reads row r's
// units from LDS in address = sample order, skipping the units of the first and the last run that belong to the neighbouring rows
// (pt_lpath_tile_has).  The other lanes only load: the kernels move 16 bytes per three additions and are bound by memory, so the shape is chosen for
// the memory side -- whole 1-KiB runs on line boundaries, PT_ACC_ROWS of them in flight per lane and no branch around a load (times under both orders:
// profiles/path_order.txt).  A row of the LDS tile is padded to PT_ACC_RUN + 1 units: rows 260 words apart fall on distinct banks
// for 16-byte reads.  Units outside [j S, (j + 1) S) and entries >= n are never loaded: nothing outside the batch's n S units is touched.
#define PT_ACC_ROWS 8u                         // entries of a wave = loads per lane and tile (PtAccRegs has one member each)
#define PT_ACC_RUN 64u                         // units (float4) of a row per tile: one load instruction of the wave
#define PT_ACC_LINE 8u                         // units of a 128-byte line: a row's runs start on a line
#define PT_ACC_ROW (PT_ACC_RUN + 1u)
#define PT_ACC_TILE_UNITS (PT_ACC_ROWS * PT_ACC_ROW)   // float4 units of one wave's tile
PT_DEV uint32_t pt_lpath_tiles(uint32_t S) { return (S + PT_ACC_LINE - 1u + PT_ACC_RUN - 1u) / PT_ACC_RUN; }   // runs a row of S units can touch
// the unit of lpath that is unit t of run k of the row starting at unit `first`, and whether it lies inside the row (its sample index is then unit - first)
PT_DEV uint32_t pt_lpath_tile_unit(uint32_t first, uint32_t k, uint32_t t) { return (first & ~(PT_ACC_LINE - 1u)) + k * PT_ACC_RUN + t; }
PT_DEV bool pt_lpath_tile_has(uint32_t first, uint32_t S, uint32_t k, uint32_t t) {
  const uint32_t e = pt_lpath_tile_unit(first, k, t);
  return e >= first && e - first < S;
}
struct PtAccRegs { float4 r0, r1, r2, r3, r4, r5, r6, r7; };      // a lane's PT_ACC_ROWS loads of a tile; named members, not an array: the array went to scratch
PT_DEV float4 pt_lpath_tile_load(const float4* __restrict__ lpath, uint32_t j, uint32_t n, uint32_t S, uint32_t k, uint32_t lane) {
  const uint32_t first = pt_path_id(PT_ORDER_PIXEL, j, 0u, n, S);
  const bool inside = j < n && pt_lpath_tile_has(first, S, k, lane);
  return lpath[inside ? pt_lpath_tile_unit(first, k, lane) : 0u];      // no branch around a load: the loads of a tile issue back to back.  Unit 0 exists (n S > 0) and nobody reads what a lane outside its row fetched
}
PT_DEV PtAccRegs pt_lpath_tile_fetch(const float4* __restrict__ lpath, uint32_t j0, uint32_t n, uint32_t S, uint32_t k, uint32_t lane) {
  PtAccRegs v;
  v.r0 = pt_lpath_tile_load(lpath, j0, n, S, k, lane); v.r1 = pt_lpath_tile_load(lpath, j0 + 1u, n, S, k, lane);
  v.r2 = pt_lpath_tile_load(lpath, j0 + 2u, n, S, k, lane); v.r3 = pt_lpath_tile_load(lpath, j0 + 3u, n, S, k, lane);
  v.r4 = pt_lpath_tile_load(lpath, j0 + 4u, n, S, k, lane); v.r5 = pt_lpath_tile_load(lpath, j0 + 5u, n, S, k, lane);
  v.r6 = pt_lpath_tile_load(lpath, j0 + 6u, n, S, k, lane); v.r7 = pt_lpath_tile_load(lpath, j0 + 7u, n, S, k, lane);
  return v;
}
PT_DEV void pt_lpath_tile_put(float4* tile, uint32_t lane, const PtAccRegs& v) {      // row i of the tile <- load i; units outside their row hold values nobody reads
  tile[lane] = v.r0; tile[PT_ACC_ROW + lane] = v.r1; tile[2u * PT_ACC_ROW + lane] = v.r2; tile[3u * PT_ACC_ROW + lane] = v.r3;
  tile[4u * PT_ACC_ROW + lane] = v.r4; tile[5u * PT_ACC_ROW + lane] = v.r5; tile[6u * PT_ACC_ROW + lane] = v.r6; tile[7u * PT_ACC_ROW + lane] = v.r7;
}
