// pt_emissive_tex.h — textured emission: glTF emissiveTexture as a light set of its own.
//
// A material may carry an emission texture and an RGB factor; its base emissive stays zero, so k_shade and the emitter table never see its primitives as emitters.
// The radiance leaving a front-facing point with texture coordinates (u, v) is Le_c = factor_c * texel_c(u, v), the texel fetched with the scene's filter mode and
// REPEAT, texel / 255 with no sRGB decode (the colour texture's convention), one-sided as P7's emission.  The set is sampled on its own once per bounce, with MIS
// against the BSDF sample only, by a pass of its own (pt_emissive_tex.hip: k_shade_emissive_tex) behind k_shade's, any(b) and the punctual pass; its terms ADD to
// theirs.  A scene without an emission texture never launches it.
//
// Everything below is the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_fma = one rounding.  The kernel, the host table
// build and the host evaluation (ptc_debug_emissive_tex_sample) call the same functions; tests/emissive_tex_reference.py restates them in numpy.
// pt_emtex_fetch is tex_fetch's arithmetic (pt_shading.h, which is device code) for the three colour channels, written for host and device.
//
// RNG: u0, r1, r2 = rng_f(key, PT_EMTEX_RNG_BASE + b + 1, 0 | 1 | 2).  k_shade uses the indices 0 .. max_bounces + 1, the other passes the bases 0x08.., 0x10.., 0x18..
// and 0x20...
//
// Weights.  w_i = A_i * max(lum(factor * m_i), 0.01 lum(factor * m_tex)): m_i the mean of the NEAREST texels at the 16 centroids of the 4x4 barycentric subdivision of
// the triangle, m_tex the mean texel of the texture.  The weights only steer variance: both MIS sides use the same pl, so the estimator is unbiased for any weights
// that leave every emitting texel drawable, which the 1 % floor does.
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"
#include "pt_scene_rules.h"

#define PT_EMTEX_RNG_BASE 0x28000000u
#define PT_EMTEX_UNITS 7u                   // float4 units of an entry
#define PT_EMTEX_FLOOR 0.01f
enum { PT_EMTEX_HITS = 0, PT_EMTEX_SHADOW = 16, PT_EMTEX_COUNTERS = 32 };      // counters, a 128-byte line each

// one entry as the kernel reads it: 112 bytes = 7 x float4
struct pt_emtex_rec {
  float p0[3]; float area;           // world vertex a; the triangle's area
  float e1[3]; float pmf;            // b - a; probability of choosing this entry
  float e2[3]; int32_t tex;          // c - a; the emission texture
  float n[3]; float pad0;            // unit face normal (zero for a degenerate triangle)
  float factor[3]; float pad1;
  float uv0[2], uv1[2];              // texture coordinates of a, b
  float uv2[2]; float pad2[2];       // ... and of c
};
static_assert(sizeof(pt_emtex_rec) == 16 * PT_EMTEX_UNITS, "pt_emtex_rec is seven 16-byte units");

// the textures as both sides hold them: RGBA8 texels back to back, four ints per texture (offset, width, height, 0), the filter mode
struct pt_emtex_textures { const uint32_t* texels; const int32_t* tex_info; int linear; };

PT_HD v3 pt_emtex_texel(const pt_emtex_textures& t, size_t at) {
  const uint32_t p = t.texels[at];
  return V3((float)(p & 255u) / 255.0f, (float)((p >> 8) & 255u) / 255.0f, (float)((p >> 16) & 255u) / 255.0f);
}
PT_HD v3 pt_emtex_fetch(const pt_emtex_textures& t, int tex, float u, float v, bool linear) {
  const int off = t.tex_info[tex * 4], w = t.tex_info[tex * 4 + 1], h = t.tex_info[tex * 4 + 2];
  const float fu = u - __builtin_floorf(u), fv = v - __builtin_floorf(v);
  if (!linear) {
    int x = (int)(fu * (float)w), y = (int)(fv * (float)h);
    if (x > w - 1) x = w - 1;
    if (y > h - 1) y = h - 1;
    return pt_emtex_texel(t, (size_t)off + (size_t)y * (size_t)w + (size_t)x);
  }
  const float x = pt_fma(fu, (float)w, -0.5f), y = pt_fma(fv, (float)h, -0.5f);
  const float x0f = __builtin_floorf(x), y0f = __builtin_floorf(y);
  const float tx = x - x0f, ty = y - y0f;
  int x0 = (int)x0f, y0 = (int)y0f;
  int x1 = x0 + 1, y1 = y0 + 1;
  if (x0 < 0) x0 += w;
  if (y0 < 0) y0 += h;
  if (x1 > w - 1) x1 -= w;
  if (y1 > h - 1) y1 -= h;
  const size_t r0 = (size_t)off + (size_t)y0 * (size_t)w, r1 = (size_t)off + (size_t)y1 * (size_t)w;
  const v3 c00 = pt_emtex_texel(t, r0 + (size_t)x0), c10 = pt_emtex_texel(t, r0 + (size_t)x1), c01 = pt_emtex_texel(t, r1 + (size_t)x0), c11 = pt_emtex_texel(t, r1 + (size_t)x1);
  const float ax = pt_fma(tx, c10.x - c00.x, c00.x), ay = pt_fma(tx, c10.y - c00.y, c00.y), az = pt_fma(tx, c10.z - c00.z, c00.z);
  const float bx = pt_fma(tx, c11.x - c01.x, c01.x), by = pt_fma(tx, c11.y - c01.y, c01.y), bz = pt_fma(tx, c11.z - c01.z, c01.z);
  return V3(pt_fma(ty, bx - ax, ax), pt_fma(ty, by - ay, ay), pt_fma(ty, bz - az, az));
}

// texture coordinates at the barycentrics (bu, bv) of (b, c): apply_textures' expression
PT_HD void pt_emtex_uv(const pt_emtex_rec& E, float bu, float bv, float& u, float& v) {
  const float bw = 1.0f - bu - bv;
  u = pt_fma(E.uv2[0], bv, pt_fma(E.uv1[0], bu, E.uv0[0] * bw));
  v = pt_fma(E.uv2[1], bv, pt_fma(E.uv1[1], bu, E.uv0[1] * bw));
}
// Le at the barycentrics (bu, bv)
PT_HD v3 pt_emtex_radiance(const pt_emtex_rec& E, const pt_emtex_textures& t, float bu, float bv) {
  float u, v;
  pt_emtex_uv(E, bu, bv, u, v);
  const v3 c = pt_emtex_fetch(t, E.tex, u, v, t.linear != 0);
  return V3(E.factor[0] * c.x, E.factor[1] * c.y, E.factor[2] * c.z);
}

// The sample of entry E seen from P with the numbers (r1, r2): k_shade's mapping of the unit square to the triangle.  y: the point, wi: the unit direction towards
// it, pl: its solid-angle density, pmf included (no p_area factor: this set is always sampled), Le: the radiance leaving y.  false: no sample (P lies on y, or sees
// the back).
PT_HD bool pt_emtex_sample(const pt_emtex_rec& E, const pt_emtex_textures& t, v3 P, float r1, float r2, v3& y, v3& wi, float& pl, v3& Le) {
  const float su = pt_sqrt(r1);
  const float bu = su * (1.0f - r2), bv = su * r2;
  y = vfma(V3(E.e2), bv, vfma(V3(E.e1), bu, V3(E.p0)));
  const v3 dv = y - P;
  const float dist2 = dot3(dv, dv);
  if (!(dist2 > 0.0f)) return false;
  float dist;
  wi = dv * pt_rnorm(dist2, dist);
  const float cosl = -dot3(V3(E.n), wi);
  if (!(cosl > 0.0f) || !(E.pmf > 0.0f)) return false;
  pl = (E.pmf * dist2) / (E.area * cosl);
  Le = pt_emtex_radiance(E, t, bu, bv);
  return true;
}
// the MIS weight of the sample against the BSDF density pb
PT_HD float pt_emtex_sample_weight(float pl, float pb) { const float pl2 = pl * pl; return pl2 / pt_fma(pb, pb, pl2); }
// the MIS weight of a front-facing hit at distance ht with cosl = dot(ng, wo), the ray's pdf word pb: 1 at bounce 0 and where the entry is never drawn
PT_HD float pt_emtex_hit_weight(const pt_emtex_rec& E, uint32_t b, float pb, float ht, float cosl) {
  if (b == 0u || E.pmf == 0.0f) return 1.0f;
  const float pl = (E.pmf * (ht * ht)) / (E.area * cosl);
  const float pb2 = pb * pb;
  return pb2 / pt_fma(pl, pl, pb2);
}

// ---- host: description -> entries, cdf, primitive map ---------------------------------------------------------------------------------------------
struct pt_emtex_material { int tex = -1; float factor[3] = {0.0f, 0.0f, 0.0f}; };

// what a commit keeps per entry (computed once): where its vertices come from, its texture coordinates, texture and factor, and the luminance term of its weight
struct pt_emtex_static { uint32_t prim; uint32_t inst; uint32_t v[3]; float uv[3][2]; int tex; float factor[3]; float lumw; };
struct pt_emtex_table {
  std::vector<pt_emtex_static> fixed;
  std::vector<pt_emtex_rec> recs;
  std::vector<float> cdf;
  std::vector<int32_t> prim_map;      // per primitive of the scene: its entry, -1: none
  float total = 0.0f;                 // 0: the pass is off
  void clear() { fixed.clear(); recs.clear(); cdf.clear(); prim_map.clear(); total = 0.0f; }
};

// the mean texel of a texture: the exact byte sums over 255 n
inline v3 pt_emtex_mean_texel(const HostTexture& T) {
  uint64_t s[3] = {0, 0, 0};
  const size_t n = (size_t)T.w * (size_t)T.h;
  for (size_t i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) s[k] += T.px[i * 4 + (size_t)k];
  const double d = 255.0 * (double)n;
  return V3((float)((double)s[0] / d), (float)((double)s[1] / d), (float)((double)s[2] / d));
}
// m_i: the 10 upright cells (i, j), i + j <= 3, then the 6 inverted ones, i + j <= 2, i outer; centroids ((i + 1/3) / 4, (j + 1/3) / 4) and ((i + 2/3) / 4, (j + 2/3) / 4)
inline v3 pt_emtex_mean_cells(const pt_emtex_rec& E, const pt_emtex_textures& t) {
  const float third = 1.0f / 3.0f, two_thirds = 2.0f / 3.0f;
  v3 s = V3(0.0f, 0.0f, 0.0f);
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < 4 - pass; ++i)
      for (int j = 0; i + j < 4 - pass; ++j) {
        const float o = pass ? two_thirds : third;
        const float bu = ((float)i + o) * 0.25f, bv = ((float)j + o) * 0.25f;
        float u, v;
        pt_emtex_uv(E, bu, bv, u, v);
        s = s + pt_emtex_fetch(t, E.tex, u, v, false);
      }
  return s * 0.0625f;
}

// The fixed part, at a commit: every primitive of a material with an emission texture, in primitive order.  texs / tex: the description's textures and the same
// texels as the committed scene holds them.
inline void pt_emtex_describe(const std::vector<pt_emtex_material>& em, const std::vector<HostMesh>& meshes, const std::vector<HostInstance>& insts, const std::vector<HostTexture>& texs,
                              const pt_emtex_textures& tex, pt_emtex_table& T) {
  T.clear();
  size_t n_tris = 0;
  bool any = false;
  for (const HostInstance& in : insts) {
    const HostMesh& m = meshes[(size_t)in.mesh];
    n_tris += m.idx.size() / 3;
    any = any || ((size_t)m.material < em.size() && em[(size_t)m.material].tex >= 0);
  }
  if (!any) return;
  T.prim_map.assign(n_tris, -1);
  std::vector<v3> mean(texs.size());
  std::vector<uint8_t> have(texs.size(), 0);
  uint32_t tb = 0;
  for (size_t i = 0; i < insts.size(); ++i) {
    const HostMesh& m = meshes[(size_t)insts[i].mesh];
    const uint32_t nt = (uint32_t)(m.idx.size() / 3);
    if ((size_t)m.material < em.size() && em[(size_t)m.material].tex >= 0) {
      const pt_emtex_material& M = em[(size_t)m.material];
      if (!have[(size_t)M.tex]) { mean[(size_t)M.tex] = pt_emtex_mean_texel(texs[(size_t)M.tex]); have[(size_t)M.tex] = 1; }
      const v3 mt = mean[(size_t)M.tex];
      const float floor_l = PT_EMTEX_FLOOR * luminance(V3(M.factor[0] * mt.x, M.factor[1] * mt.y, M.factor[2] * mt.z));
      for (uint32_t k = 0; k < nt; ++k) {
        pt_emtex_static s{};
        s.prim = tb + k; s.inst = (uint32_t)i; s.tex = M.tex;
        pt_emtex_rec E{};
        E.tex = M.tex;
        for (int c = 0; c < 3; ++c) {
          s.v[c] = m.idx[(size_t)k * 3 + (size_t)c];
          s.factor[c] = M.factor[c];
          s.uv[c][0] = m.v[s.v[c]].texcoord[0]; s.uv[c][1] = m.v[s.v[c]].texcoord[1];
        }
        E.uv0[0] = s.uv[0][0]; E.uv0[1] = s.uv[0][1]; E.uv1[0] = s.uv[1][0]; E.uv1[1] = s.uv[1][1]; E.uv2[0] = s.uv[2][0]; E.uv2[1] = s.uv[2][1];
        const v3 mi = pt_emtex_mean_cells(E, tex);
        s.lumw = fmax2(luminance(V3(M.factor[0] * mi.x, M.factor[1] * mi.y, M.factor[2] * mi.z)), floor_l);
        T.prim_map[s.prim] = (int32_t)T.fixed.size();
        T.fixed.push_back(s);
      }
    }
    tb += nt;
  }
}

// The moving part, at a commit, a refit and a rebuild: world geometry, areas, pmf and cdf from these primitives' vertices alone, each taken through its instance's
// matrix with the flatten's expression; pmf and cdf as ptc_scene.cpp builds the emitter cdf (binary32 running sums, cdf[i] = run / total, last entry 1)
inline void pt_emtex_place(const std::vector<HostMesh>& meshes, const std::vector<HostInstance>& insts, pt_emtex_table& T) {
  const size_t n = T.fixed.size();
  T.recs.assign(n, pt_emtex_rec{});
  T.cdf.assign(n, 0.0f);
  std::vector<float> weight(n, 0.0f);
  for (size_t j = 0; j < n; ++j) {
    const pt_emtex_static& s = T.fixed[j];
    const HostInstance& in = insts[s.inst];
    const HostMesh& mesh = meshes[(size_t)in.mesh];
    float w[3][3];
    for (int c = 0; c < 3; ++c) scene_rules::store3(w[c], scene_rules::transform_point(in.m, 4, V3(mesh.v[s.v[c]].position)));
    const float *a = w[0], *b = w[1], *cc = w[2];
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
    const v3 cr = cross3(V3(e1), V3(e2));
    const float len = pt_sqrt(dot3(cr, cr));
    const float area = 0.5f * len;
    pt_emtex_rec& E = T.recs[j];
    for (int k = 0; k < 3; ++k) { E.p0[k] = a[k]; E.e1[k] = e1[k]; E.e2[k] = e2[k]; E.factor[k] = s.factor[k]; }
    E.area = area; E.tex = s.tex;
    E.uv0[0] = s.uv[0][0]; E.uv0[1] = s.uv[0][1]; E.uv1[0] = s.uv[1][0]; E.uv1[1] = s.uv[1][1]; E.uv2[0] = s.uv[2][0]; E.uv2[1] = s.uv[2][1];
    const float wgt = area * s.lumw;
    if (len > 0.0f && len - len == 0.0f && wgt - wgt == 0.0f) {      // a degenerate or non-finite triangle keeps weight 0 and a zero normal: never drawn
      const float il = 1.0f / len;
      E.n[0] = cr.x * il; E.n[1] = cr.y * il; E.n[2] = cr.z * il;
      weight[j] = wgt;
    } else E.area = 0.0f;
  }
  float total = 0.0f;
  for (float wv : weight) total += wv;
  T.total = total > 0.0f ? total : 0.0f;
  if (!(total > 0.0f)) return;
  float run = 0.0f;
  for (size_t j = 0; j < n; ++j) {
    run += weight[j];
    T.cdf[j] = run / total;
    T.recs[j].pmf = weight[j] / total;
  }
  size_t last = n - 1;
  while (last > 0 && !(weight[last] > 0.0f)) --last;      // entries of weight 0 behind the last one that has weight: never drawn either
  for (size_t j = last; j < n; ++j) T.cdf[j] = 1.0f;
}

// ---- the kernel (pt_emissive_tex.hip) -----------------------------------------------------------------------------------------------------------------
struct DevEmTex {
  const float4* recs;                 // n entries of PT_EMTEX_UNITS units
  const float* cdf;                   // n
  const int32_t* prim_map;            // per primitive: entry or -1
  uint32_t n;
  int sample;                         // the table has weight: the sample side runs
  unsigned long long* counters;       // PT_EMTEX_COUNTERS words
};
// k_shade_emissive_tex: the pass of bounce b over the rays of ray[qi] and their hit records, as k_shade(b) read them.  It adds the hit side to q.lpath and — when
// b < max_bounces and the table has weight — writes shadow records to the front of each segment of q.shadow and their number to q.seg_sh; nothing else.
void pt_launch_shade_emissive_tex(hipStream_t, const DevScene&, const DevQueues&, int qi, uint32_t bounce, uint32_t max_bounces, const DevEmTex&);
