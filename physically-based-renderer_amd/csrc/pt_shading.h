// pt_shading.h — what two translation units need of a hit's surface: the hit word, the loaders, the texture fetch and P5 (device only).
//
// k_shade, k_shade_raster and k_guides (pt_kernels.hip) and k_shade_punctual (pt_lights.hip) rebuild the surface of a hit from the same shading record, the same
// material and the same texels.  The helpers are templates over the scene type: k_shade passes its GScene (arrays typed as global memory), the kernels that
// receive a DevScene by value pass that.
#pragma once
#include "pt_device.h"
#include "ptc_internal.h"

#define HIT_CLASS_SHIFT 28

typedef float fx4 __attribute__((ext_vector_type(4)));
typedef uint32_t ux4 __attribute__((ext_vector_type(4)));
typedef int ix4 __attribute__((ext_vector_type(4)));
#define AS_GLOBAL __attribute__((address_space(1)))
#define AS_LDS __attribute__((address_space(3)))
PT_DEV float4 ld4(const float4* p, size_t i) { return p[i]; }
PT_DEV float4 ld4(AS_GLOBAL const fx4* p, size_t i) { const fx4 v = p[i]; return make_float4(v.x, v.y, v.z, v.w); }
PT_DEV float4 ld4(AS_LDS const fx4* p, size_t i) { const fx4 v = p[i]; return make_float4(v.x, v.y, v.z, v.w); }
PT_DEV uint4 ldu4(const uint4* p, size_t i) { return p[i]; }
PT_DEV uint4 ldu4(AS_GLOBAL const ux4* p, size_t i) { const ux4 v = p[i]; return make_uint4(v.x, v.y, v.z, v.w); }
PT_DEV int4 ldi4(const int4* p, size_t i) { return p[i]; }
PT_DEV int4 ldi4(AS_GLOBAL const ix4* p, size_t i) { const ix4 v = p[i]; return make_int4(v.x, v.y, v.z, v.w); }

// R7 sampler: NEAREST, REPEAT, no mips (the reference creates its samplers with default create-info, gltf/Asset.cpp:116-117);
// RGBA8 UNORM texel → float / 255.
template <class S> PT_DEV float4 texel_rgba(const S& sc, size_t at) {
  const uint32_t p = sc.texels[at];
  return make_float4((float)(p & 255u) / 255.0f, (float)((p >> 8) & 255u) / 255.0f, (float)((p >> 16) & 255u) / 255.0f, (float)(p >> 24) / 255.0f);
}
template <class S> PT_DEV float4 tex_fetch(const S& sc, int tex, float u, float v) {
  const int4 ti = ldi4(sc.tex_info, (size_t)tex);
  const float fu = u - __builtin_floorf(u), fv = v - __builtin_floorf(v);
  if (!sc.tex_linear) {
    int x = (int)(fu * (float)ti.y), y = (int)(fv * (float)ti.z);
    if (x > ti.y - 1) x = ti.y - 1;
    if (y > ti.z - 1) y = ti.z - 1;
    return texel_rgba(sc, (size_t)ti.x + (size_t)y * (size_t)ti.y + (size_t)x);
  }
  // PTC_FILTER_LINEAR: texel centres at i + 0.5, REPEAT wrap, lerp(a, b, t) = fma(t, b - a, a), x then y
  const float x = pt_fma(fu, (float)ti.y, -0.5f), y = pt_fma(fv, (float)ti.z, -0.5f);
  const float x0f = __builtin_floorf(x), y0f = __builtin_floorf(y);
  const float tx = x - x0f, ty = y - y0f;
  int x0 = (int)x0f, y0 = (int)y0f;
  int x1 = x0 + 1, y1 = y0 + 1;
  if (x0 < 0) x0 += ti.y;
  if (y0 < 0) y0 += ti.z;
  if (x1 > ti.y - 1) x1 -= ti.y;
  if (y1 > ti.z - 1) y1 -= ti.z;
  const size_t r0 = (size_t)ti.x + (size_t)y0 * (size_t)ti.y, r1 = (size_t)ti.x + (size_t)y1 * (size_t)ti.y;
  const float4 c00 = texel_rgba(sc, r0 + (size_t)x0), c10 = texel_rgba(sc, r0 + (size_t)x1), c01 = texel_rgba(sc, r1 + (size_t)x0), c11 = texel_rgba(sc, r1 + (size_t)x1);
  const float ax = pt_fma(tx, c10.x - c00.x, c00.x), ay = pt_fma(tx, c10.y - c00.y, c00.y), az = pt_fma(tx, c10.z - c00.z, c00.z), aw = pt_fma(tx, c10.w - c00.w, c00.w);
  const float bx = pt_fma(tx, c11.x - c01.x, c01.x), by = pt_fma(tx, c11.y - c01.y, c01.y), bz = pt_fma(tx, c11.z - c01.z, c01.z), bw = pt_fma(tx, c11.w - c01.w, c01.w);
  return make_float4(pt_fma(ty, bx - ax, ax), pt_fma(ty, by - ay, ay), pt_fma(ty, bz - az, az), pt_fma(ty, bw - aw, aw));
}

// Texel address inside a texture set: 8x8 tiles row-major over the image, Morton order inside a tile (ptc_scene.cpp).
PT_DEV size_t set_texel_at(int4 si, int x, int y) {
  const uint32_t lx = (uint32_t)x & 7u, ly = (uint32_t)y & 7u;
  const uint32_t mo = (lx & 1u) | ((ly & 1u) << 1) | ((lx & 2u) << 1) | ((ly & 2u) << 2) | ((lx & 4u) << 2) | ((ly & 4u) << 3);
  return (size_t)si.x + ((size_t)((uint32_t)y >> 3) * (size_t)si.w + ((uint32_t)x >> 3)) * 64u + mo;
}
PT_DEV float4 unorm8x4(uint32_t p) {
  return make_float4((float)(p & 255u) / 255.0f, (float)((p >> 8) & 255u) / 255.0f, (float)((p >> 16) & 255u) / 255.0f, (float)(p >> 24) / 255.0f);
}
// The three texels (colour, normal, metal-rough) of a texture set at (u, v): ONE 16-byte gather per tap instead of three 4-byte gathers from
// three textures.  Same arithmetic per texture as tex_fetch (the set's textures share one size, so the tap coordinates are the same).
template <class S> PT_DEV void set_fetch(const S& sc, int4 si, float u, float v, float4& c, float4& n, float4& m) {
  const float fu = u - __builtin_floorf(u), fv = v - __builtin_floorf(v);
  if (!sc.tex_linear) {
    int x = (int)(fu * (float)si.y), y = (int)(fv * (float)si.z);
    if (x > si.y - 1) x = si.y - 1;
    if (y > si.z - 1) y = si.z - 1;
    const uint4 t = ldu4(sc.set_texels, set_texel_at(si, x, y));
    c = unorm8x4(t.x); n = unorm8x4(t.y); m = unorm8x4(t.z);
    return;
  }
  const float x = pt_fma(fu, (float)si.y, -0.5f), y = pt_fma(fv, (float)si.z, -0.5f);
  const float x0f = __builtin_floorf(x), y0f = __builtin_floorf(y);
  const float tx = x - x0f, ty = y - y0f;
  int x0 = (int)x0f, y0 = (int)y0f;
  int x1 = x0 + 1, y1 = y0 + 1;
  if (x0 < 0) x0 += si.y;
  if (y0 < 0) y0 += si.z;
  if (x1 > si.y - 1) x1 -= si.y;
  if (y1 > si.z - 1) y1 -= si.z;
  const uint4 t00 = ldu4(sc.set_texels, set_texel_at(si, x0, y0)), t10 = ldu4(sc.set_texels, set_texel_at(si, x1, y0)),
              t01 = ldu4(sc.set_texels, set_texel_at(si, x0, y1)), t11 = ldu4(sc.set_texels, set_texel_at(si, x1, y1));
  auto bil = [&](uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11) {
    const float4 c00 = unorm8x4(p00), c10 = unorm8x4(p10), c01 = unorm8x4(p01), c11 = unorm8x4(p11);
    const float ax = pt_fma(tx, c10.x - c00.x, c00.x), ay = pt_fma(tx, c10.y - c00.y, c00.y), az = pt_fma(tx, c10.z - c00.z, c00.z), aw = pt_fma(tx, c10.w - c00.w, c00.w);
    const float bx = pt_fma(tx, c11.x - c01.x, c01.x), by = pt_fma(tx, c11.y - c01.y, c01.y), bz = pt_fma(tx, c11.z - c01.z, c01.z), bw = pt_fma(tx, c11.w - c01.w, c01.w);
    return make_float4(pt_fma(ty, bx - ax, ax), pt_fma(ty, by - ay, ay), pt_fma(ty, bz - az, az), pt_fma(ty, bw - aw, aw));
  };
  c = bil(t00.x, t10.x, t01.x, t11.x); n = bil(t00.y, t10.y, t01.y, t11.y); m = bil(t00.z, t10.z, t01.z, t11.z);
}

// Textured surface attributes of primitive `prim` at barycentrics (hu, hv): base colour × texel, metallic-roughness texel
// (glTF: G = roughness, B = metallic), tangent-space normal map through the interpolated TBN (fragment.glsl:24-30).
// ni = interpolated (un-normalised) vertex normal.  Updates base/metallic/roughness/ns in place.  `set` is the material's texture
// set (M3.x): when the set has an interleaved copy the three texels come with one gather, else one fetch per texture.
template <class S> PT_DEV void apply_textures(const S& sc, float4 t0, float4 t1, float4 t2, float4 t3, float4 t4, float4 t5, float hu, float hv, float hw, float4 M2, int set, v3 ni, float base[4],
                           float& metallic, float& roughness, v3& ns) {
  const int tex_color = __float_as_int(M2.y), tex_normal = __float_as_int(M2.z), tex_mr = __float_as_int(M2.w);
  const float tu = pt_fma(t1.x, hv, pt_fma(t0.z, hu, t0.x * hw)), tv = pt_fma(t1.y, hv, pt_fma(t0.w, hu, t0.y * hw));
  float4 cc = make_float4(1, 1, 1, 1), cn = make_float4(0.5f, 0.5f, 1.0f, 1.0f), cm = make_float4(1, 1, 1, 1);
  const int4 si = ldi4(sc.set_info, (size_t)(set < 0 ? 0 : set));
  if (set >= 0 && si.x >= 0) set_fetch(sc, si, tu, tv, cc, cn, cm);
  else {
    if (tex_color >= 0) cc = tex_fetch(sc, tex_color, tu, tv);
    if (tex_mr >= 0) cm = tex_fetch(sc, tex_mr, tu, tv);
    if (tex_normal >= 0) cn = tex_fetch(sc, tex_normal, tu, tv);
  }
  if (tex_color >= 0) { base[0] = base[0] * cc.x; base[1] = base[1] * cc.y; base[2] = base[2] * cc.z; base[3] = base[3] * cc.w; }
  if (tex_mr >= 0) { roughness = roughness * cm.y; metallic = metallic * cm.z; }
  if (tex_normal >= 0) {
    const float nx = 2.0f * cn.x - 1.0f, ny = 2.0f * cn.y - 1.0f, nz = 2.0f * cn.z - 1.0f;
    // tangents: a = (t1.z, t1.w, t2.x) b = (t2.y, t2.z, t2.w) c = (t3.x, t3.y, t3.z); bitangents: a = (t3.w, t4.x, t4.y) b = (t4.z, t4.w, t5.x) c = (t5.y, t5.z, t5.w)
    const v3 ti = V3(pt_fma(t3.x, hv, pt_fma(t2.y, hu, t1.z * hw)), pt_fma(t3.y, hv, pt_fma(t2.z, hu, t1.w * hw)), pt_fma(t3.z, hv, pt_fma(t2.w, hu, t2.x * hw)));
    const v3 bi = V3(pt_fma(t5.y, hv, pt_fma(t4.z, hu, t3.w * hw)), pt_fma(t5.z, hv, pt_fma(t4.w, hu, t4.x * hw)), pt_fma(t5.w, hv, pt_fma(t5.x, hu, t4.y * hw)));
    ns = normalize3(vfma(ti, nx, vfma(bi, ny, ni * nz)));
  }
}

template <class P> PT_DEV uint32_t cdf_search(const P& cdf, uint32_t n, float r) {
  uint32_t lo = 0, hi = n - 1u;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cdf[mid] > r) hi = mid; else lo = mid + 1u; }
  return lo;
}

// ---- P5: the surface of a hit, from units of the primitive's shading record that the caller has ALREADY loaded (so every kernel keeps its own load order) ----
// units 0..4: positions a b c (r0.xyz r1.xyz r2.xyz), vertex normals a b c (r2.w .. r4.w), r0.w the material, r1.w the emitter; (hw, hu, hv) weigh (a, b, c).
PT_DEV v3 record_position(float4 r0, float4 r1, float4 r2, float hu, float hv, float hw) {
  return V3(pt_fma(r2.x, hv, pt_fma(r1.x, hu, r0.x * hw)), pt_fma(r2.y, hv, pt_fma(r1.y, hu, r0.y * hw)), pt_fma(r2.z, hv, pt_fma(r1.z, hu, r0.z * hw)));
}
PT_DEV v3 record_face_normal(float4 r0, float4 r1, float4 r2) {
  const v3 Pa = V3(r0.x, r0.y, r0.z), Pb = V3(r1.x, r1.y, r1.z), Pc = V3(r2.x, r2.y, r2.z);
  return normalize3(cross3(Pb - Pa, Pc - Pa));
}
// the interpolated vertex normal, not normalised: what apply_textures takes as ni
PT_DEV v3 record_normal(float4 r2, float4 r3, float4 r4, float hu, float hv, float hw) {
  return V3(pt_fma(r4.y, hv, pt_fma(r3.z, hu, r2.w * hw)), pt_fma(r4.z, hv, pt_fma(r3.w, hu, r3.x * hw)), pt_fma(r4.w, hv, pt_fma(r4.x, hu, r3.y * hw)));
}
// Material `mat` of the table `mats` at the hit: base colour, metallic, roughness and — for a textured material, x0..x5 being the record's units 5..10 — the
// texels applied and ns replaced by the mapped normal.  lambert: whether the material is of the Lambert class.
template <class S, class M> PT_DEV void record_material(const S& sc, const M& mats, int mat, float4 x0, float4 x1, float4 x2, float4 x3, float4 x4, float4 x5, float hu, float hv, float hw,
                                                        v3 ni, float base[4], float& metallic, float& roughness, bool& lambert, v3& ns) {
  const float4 M0 = ld4(mats, (size_t)(mat * 4 + 0)), M1 = ld4(mats, (size_t)(mat * 4 + 1)), M2 = ld4(mats, (size_t)(mat * 4 + 2));
  base[0] = M0.x; base[1] = M0.y; base[2] = M0.z; base[3] = M2.x;
  metallic = M0.w; roughness = M1.w;
  lambert = metallic == 0.0f && roughness >= 1.0f && __float_as_int(M2.w) < 0;
  if (__float_as_int(M2.y) >= 0 || __float_as_int(M2.z) >= 0 || __float_as_int(M2.w) >= 0)
    apply_textures(sc, x0, x1, x2, x3, x4, x5, hu, hv, hw, M2, __float_as_int(ld4(mats, (size_t)(mat * 4 + 3)).x), ni, base, metallic, roughness, ns);
}
// ng and ns turned to the side wo lies on; a shading normal that still looks away from wo gives way to ng.  Returns whether wo sees the front face.
PT_DEV bool orient_normals(v3 wo, v3& ng, v3& ns) {
  const bool front = dot3(ng, wo) > 0.0f;
  if (dot3(ns, ng) < 0.0f) ns = -ns;
  if (!front) { ng = -ng; ns = -ns; }
  if (!(dot3(ns, wo) > 0.0f)) ns = ng;
  return front;
}
