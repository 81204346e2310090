// pt_lightmap.h — lightmaps: path-traced irradiance on the surfaces of one instance, over the texels of its UV atlas.
//
// A lightmap frame is a frame of the path integrator whose "pixels" are the covered texels of the atlas: it has a front of its own (the UV triangles rasterised
// into texels, an oriented ray per texel and sample) and a back of its own (the count of back-face first hits, the resolve into the atlas, the dilation of the
// gutters); nothing between the two knows that a path did not come from a camera, and k_accumulate's ordered per-entry sum is the accumulator: with
// cosine-weighted directions the irradiance is pi x mean(L).  The functions below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in
// the order written, pt_fma = one rounding; coverage is integer arithmetic and exact.  The host evaluation (ptc_debug_lightmap_cover / _rays / _dilate on a
// description-only context) and the kernels (pt_lightmap.hip) both call them, so the device computes the bytes the host computes.
// tests/lightmap_reference.py restates them in numpy.
//
// path_key, rng_f and sincos2pi are pt_device.h's host + device functions.
//
// Coverage: UVs are clamped to [0, 1] and go to fixed point with 8 sub-texel bits; texel (x, y) has its centre at ((2x + 1) 128, (2y + 1) 128).  Coordinates
// are at most 2^21 and every product below 2^44: the three edge functions and the doubled area are exact in int64.  A triangle of zero UV area covers nothing;
// another covers every centre whose three edge values, oriented by the sign of the area, are >= 0 (inclusive: two triangles that share an edge leave no centre
// on it unowned), and the owner of a texel is the LOWEST primitive index that covers it — a minimum, which no order of evaluation changes.
//
// RNG dimensions: a texel has no pixel jitter, so dimensions 0 and 1 of the path's RNG index 0 are free, as for probes; the direction takes them.  The key of
// atlas index a, sample s is path_key(seed_hash, base + a, s): by atlas index, not by list entry, so that a texel's result does not depend on what else is
// covered and shards of an atlas concatenate.
#pragma once
#include "ptc_internal.h"
#include "pt_device.h"

#define PT_LM_MAX_SIDE 8192            // texels per side: W H <= 2^26
#define PT_LM_SUB 256                  // sub-texel steps per texel
#define PT_LM_NONE 0xffffffffu         // owner image: no primitive covers the texel
#define PT_LM_PI 3.1415927f
#define PT_LM_MAX_DILATE 64

// ---- coverage -----------------------------------------------------------------------------------------------------------------------------------
struct pt_lm_tri { int32_t x[3], y[3]; int64_t area; };      // fixed-point corners and the doubled signed area

PT_HD int32_t pt_lm_fixed(float u, int side) {
  const float c = fmin2(fmax2(u, 0.0f), 1.0f);
  return (int32_t)__builtin_rintf((c * (float)side) * (float)PT_LM_SUB);
}
PT_HD int64_t pt_lm_orient(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t cx, int32_t cy) {
  return (int64_t)(bx - ax) * (int64_t)(cy - ay) - (int64_t)(by - ay) * (int64_t)(cx - ax);
}
PT_HD pt_lm_tri pt_lm_make_tri(const float uv0[2], const float uv1[2], const float uv2[2], int w, int h) {
  pt_lm_tri t;
  t.x[0] = pt_lm_fixed(uv0[0], w); t.y[0] = pt_lm_fixed(uv0[1], h);
  t.x[1] = pt_lm_fixed(uv1[0], w); t.y[1] = pt_lm_fixed(uv1[1], h);
  t.x[2] = pt_lm_fixed(uv2[0], w); t.y[2] = pt_lm_fixed(uv2[1], h);
  t.area = pt_lm_orient(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
  return t;
}
// the texels whose centres lie inside the triangle's bounding box, clamped to the atlas: x0 > x1 or y0 > y1 when there is none
PT_HD void pt_lm_box(const pt_lm_tri& t, int w, int h, int& x0, int& x1, int& y0, int& y1) {
  const int32_t lx = t.x[0] < t.x[1] ? (t.x[0] < t.x[2] ? t.x[0] : t.x[2]) : (t.x[1] < t.x[2] ? t.x[1] : t.x[2]);
  const int32_t hx = t.x[0] > t.x[1] ? (t.x[0] > t.x[2] ? t.x[0] : t.x[2]) : (t.x[1] > t.x[2] ? t.x[1] : t.x[2]);
  const int32_t ly = t.y[0] < t.y[1] ? (t.y[0] < t.y[2] ? t.y[0] : t.y[2]) : (t.y[1] < t.y[2] ? t.y[1] : t.y[2]);
  const int32_t hy = t.y[0] > t.y[1] ? (t.y[0] > t.y[2] ? t.y[0] : t.y[2]) : (t.y[1] > t.y[2] ? t.y[1] : t.y[2]);
  // centre (2x + 1) 128 >= l  <=>  x >= (l - 128) / 256 rounded up; <= h  <=>  x <= (h - 128) / 256 rounded down (an arithmetic shift: h - 128 may be negative)
  x0 = (lx + 127) >> 8; x1 = (hx - 128) >> 8;
  y0 = (ly + 127) >> 8; y1 = (hy - 128) >> 8;
  if (x1 > w - 1) x1 = w - 1;
  if (y1 > h - 1) y1 = h - 1;
}
// the three edge values at the centre of texel (x, y), oriented by the sign of the area (e[k] lies opposite corner k, their sum is |area|); true: covered
PT_HD bool pt_lm_edges(const pt_lm_tri& t, int x, int y, int64_t e[3]) {
  const int32_t px = (2 * x + 1) * (PT_LM_SUB / 2), py = (2 * y + 1) * (PT_LM_SUB / 2);
  int64_t e0 = pt_lm_orient(t.x[1], t.y[1], t.x[2], t.y[2], px, py);
  int64_t e1 = pt_lm_orient(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
  int64_t e2 = pt_lm_orient(t.x[0], t.y[0], t.x[1], t.y[1], px, py);
  if (t.area < 0) { e0 = -e0; e1 = -e1; e2 = -e2; }
  e[0] = e0; e[1] = e1; e[2] = e2;
  return t.area != 0 && e0 >= 0 && e1 >= 0 && e2 >= 0;
}

// ---- the texel record ---------------------------------------------------------------------------------------------------------------------------
PT_HD bool pt_lm_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
PT_HD bool pt_lm_finite3(v3 a) { return pt_lm_finite(a.x) && pt_lm_finite(a.y) && pt_lm_finite(a.z); }
// the unit face normal of the world triangle; not finite when its area is zero: such a texel is dropped from the list
PT_HD v3 pt_lm_face_normal(v3 p0, v3 p1, v3 p2) { return normalize3(cross3(p1 - p0, p2 - p0)); }
PT_HD v3 pt_lm_bary(v3 a0, v3 a1, v3 a2, float w0, float w1, float w2) {
  return V3(pt_fma(a2.x, w2, pt_fma(a1.x, w1, a0.x * w0)), pt_fma(a2.y, w2, pt_fma(a1.y, w1, a0.y * w0)), pt_fma(a2.z, w2, pt_fma(a1.z, w1, a0.z * w0)));
}
// origin and hemisphere normal of the texel whose owner has the oriented edge values e at its centre; world positions p and normals n of the owner's corners
PT_HD void pt_lm_texel(const int64_t e[3], v3 p0, v3 p1, v3 p2, v3 n0, v3 n1, v3 n2, float ray_eps, v3& origin, v3& normal) {
  const int64_t A = e[0] + e[1] + e[2];
  const float fA = (float)A;
  const float w0 = (float)e[0] / fA, w1 = (float)e[1] / fA, w2 = (1.0f - w0) - w1;
  const v3 P = pt_lm_bary(p0, p1, p2, w0, w1, w2);
  const v3 ng = pt_lm_face_normal(p0, p1, p2);
  v3 ns = normalize3(pt_lm_bary(n0, n1, n2, w0, w1, w2));
  if (!pt_lm_finite3(ns)) ns = ng;
  const v3 ngo = dot3(ng, ns) < 0.0f ? -ng : ng;
  origin = vfma(ngo, ray_eps, P);
  normal = ns;
}

// ---- the ray ------------------------------------------------------------------------------------------------------------------------------------
// k_shade's basis around a normal (pt_device.h: onb, Duff et al. 2017), for host and device
PT_HD void pt_lm_onb(v3 n, v3& t, v3& b) {
  float sg = __builtin_copysignf(1.0f, n.z);
  float a = -1.0f / (sg + n.z);
  float bb = n.x * n.y * a;
  t = V3(pt_fma(sg * n.x, n.x * a, 1.0f), sg * bb, -sg * n.x);
  b = V3(bb, pt_fma(n.y, n.y * a, sg), -n.y);
}
// The ray of (atlas index `idx` = base + a, sample) around the unit normal n: unit direction d, cosine-weighted over the hemisphere of n, and the path's RNG key
PT_HD void pt_lm_dir(uint32_t seed_hash, uint32_t idx, uint32_t sample, v3 n, float d[3], uint32_t& key_out) {
  const uint32_t key = path_key(seed_hash, idx, sample);
  const float u1 = rng_f(key, 0, 0), u2 = rng_f(key, 0, 1);
  const float r = __builtin_sqrtf(u1), z = __builtin_sqrtf(__builtin_fmaxf(1.0f - u1, 0.0f));
  float sn, co; sincos2pi(u2, sn, co);
  v3 tx, ty; pt_lm_onb(n, tx, ty);
  const v3 v = vfma(tx, r * co, vfma(ty, r * sn, n * z));
  const float inv = 1.0f / __builtin_sqrtf(pt_fma(v.z, v.z, pt_fma(v.y, v.y, v.x * v.x)));      // the camera ray's normalisation
  d[0] = v.x * inv; d[1] = v.y * inv; d[2] = v.z * inv;
  key_out = key;
}

// ---- resolve, validity, dilation ------------------------------------------------------------------------------------------------------------------
// E = sum * (pi / N), N the samples accumulated (or the resolve divisor of a sample-range shard)
PT_HD float pt_lm_resolve_scale(uint32_t n_samples) { return PT_LM_PI / (float)n_samples; }
// an entry whose first hits were back faces in more than `threshold` of its samples lies inside geometry; threshold >= 1 switches the test off
PT_HD bool pt_lm_invalid(uint32_t back, uint32_t n_samples, float threshold) { return (float)back > threshold * (float)n_samples; }
// One dilation step for texel (x, y) of a w x h RGBA image whose alpha is 1 (baked), 0.5 (filled) or 0 (empty): a non-empty texel keeps its value; an empty one
// with non-empty neighbours among its 8 takes the mean of their RGB (summed in the order written, one division by the count) and alpha 0.5
PT_HD float4 pt_lm_dilate(const float4* in, int w, int h, int x, int y) {
  const float4 c = in[(size_t)y * (size_t)w + (size_t)x];
  if (c.w != 0.0f) return c;
  const int dx[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, dy[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
  float sr = 0.0f, sg = 0.0f, sb = 0.0f;
  int cnt = 0;
  for (int k = 0; k < 8; ++k) {
    const int xx = x + dx[k], yy = y + dy[k];
    if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
    const float4 q = in[(size_t)yy * (size_t)w + (size_t)xx];
    if (q.w == 0.0f) continue;
    sr = sr + q.x; sg = sg + q.y; sb = sb + q.z; ++cnt;
  }
  if (!cnt) return c;
  const float fc = (float)cnt;
  return make_float4(sr / fc, sg / fc, sb / fc, 0.5f);
}

// ---- the kernels (pt_lightmap.hip) ------------------------------------------------------------------------------------------------------------------
// The geometry of the instance being baked: its world vertices (verts[0] is the instance's first), the world-vertex indices of its n_tris primitives (3 each,
// counted over the whole scene: vert_first is subtracted), and 2 floats of atlas UV per vertex
struct DevLmGeom { const HostVertex* verts; const uint32_t* widx; uint32_t vert_first; const float* uv; uint32_t n_tris; int w, h; };
// the scratch of the texel-list build: a flag byte per texel, the per-block counts of the stable compaction (pt_lm_blocks(w h) words), and two words: the list's
// length and the number of owned texels dropped for a degenerate world triangle
struct DevLmScratch { uint8_t* flags; uint32_t* block_tot; uint32_t* counts; };
#define PT_LM_BLOCK 256u
inline uint32_t pt_lm_blocks(uint32_t n) { return (n + PT_LM_BLOCK - 1u) / PT_LM_BLOCK; }
// k_lm_cover: owner (w h words) <- PT_LM_NONE, then the lowest covering primitive per texel
void pt_launch_lm_cover(hipStream_t, const DevLmGeom&, uint32_t* owner);
// flags + stable compaction: list <- the owned texels whose world triangle has a finite face normal, in ascending atlas index (list holds w h words); when the
// stream has run, counts[0] is the list's length and counts[1] the number of owned texels dropped
void pt_launch_lm_list(hipStream_t, const DevLmGeom&, const uint32_t* owner, const DevLmScratch&, uint32_t* list);
// k_lm_texels: two float4 per entry of the list, (origin, atlas index bits) (normal, primitive bits)
void pt_launch_lm_texels(hipStream_t, const DevLmGeom&, const uint32_t* owner, const uint32_t* list, uint32_t n_entries, float ray_eps, float4* texels);
// k_raygen_texel: pt_launch_raygen's job for a lightmap frame — path p is entry e = p % n, sample first_sample + p / n; k_raygen's queue record
void pt_launch_raygen_texel(hipStream_t, const float4* texels, uint32_t n_entries, uint32_t index_base, uint32_t seed_hash, const DevQueues&, uint32_t first_sample, uint32_t n_samples);
// k_lm_first_hit: over the live slots of ray[qi] and their hit records, back[path % n] += 1 for a hit whose face normal looks along the ray
void pt_launch_lm_first_hit(hipStream_t, const DevScene&, const DevQueues&, int qi, uint32_t n_entries, uint32_t* back);
// k_lm_scatter: atlas[atlas index of e] = (sum_e * (pi / N), 1), or empty for an invalid entry; out_back (or null): back_e / N per entry.  The atlas is cleared by the caller
void pt_launch_lm_scatter(hipStream_t, const float4* texels, uint32_t n_entries, const float4* accum, const uint32_t* back, uint32_t n_samples, float threshold, float4* atlas, float* out_back);
// k_lm_dilate: one iteration, in -> out
void pt_launch_lm_dilate(hipStream_t, const float4* in, float4* out, int w, int h);
