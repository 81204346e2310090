// pt_scene_rules.h — the rules that turn a scene description into the bytes in HBM, written once for the host builder (ptc_scene.cpp) and the device builders
// (pt_refit.hip, pt_build.hip).  The contract between the builders is byte equality of the result (tests/test_gpu_parity.py, tests/test_gpu_device_sah.py,
// tools/fuzz_parity.py), and it holds because both sides run THIS text under pt_device.h's arithmetic contract (no contraction, correctly rounded / and sqrt).
// Every function computes a value from values: no containers, no scene state, no wave intrinsics.  Who computes which value — the host's sequential loops, a
// lane of an octet, a wave scan — is the caller's business; the layout and numbering algorithms, the sorts and the sweeps stay with the callers.
#pragma once
#include "pt_device.h"
#include "ptc_internal.h"

#define PTC_SA_COST_ONE 1048576.0f                    // ptc_stats.bvh_sa_cost is summed in units of 2^-20

namespace scene_rules {
constexpr int kWide = 8;                              // child slots per BVH node
constexpr int kLeafMax = PT_LEAF_MAX;                 // triangles per leaf
constexpr int kSahBins = 32;                          // bins per axis of a binned surface-area split
constexpr float kGridCells = 65535.0f;                // node origins are 16 bits per axis on a grid over the scene box
constexpr float kCostNode = 1.0f, kCostPrim = 1.0f;   // surface-area cost of one node visit / one triangle test (collapse)

// ---- instance transform (R3, R4): world position, normal, tangent and bitangent (vertex.glsl:28-40) of an object-space vertex -------------------------
// m: rows 0..2 of the column-major model matrix, `col` floats from one column to the next; N: the 3x3 normal matrix, column-major
PT_HD v3 transform_point(const float* m, int col, v3 p) {
  return V3(m[0] * p.x + m[col] * p.y + m[2 * col] * p.z + m[3 * col], m[1] * p.x + m[col + 1] * p.y + m[2 * col + 1] * p.z + m[3 * col + 1],
            m[2] * p.x + m[col + 2] * p.y + m[2 * col + 2] * p.z + m[3 * col + 2]);
}
PT_HD v3 mul_n(const float* N, v3 v) {
  return V3(N[0] * v.x + N[3] * v.y + N[6] * v.z, N[1] * v.x + N[4] * v.y + N[7] * v.z, N[2] * v.x + N[5] * v.y + N[8] * v.z);
}
PT_HD void store3(float* o, v3 a) { o[0] = a.x; o[1] = a.y; o[2] = a.z; }
PT_HD HostVertex world_vertex(const float* m, int col, const float* N, const HostVertex& s, float bt[3]) {
  HostVertex d;
  store3(d.position, transform_point(m, col, V3(s.position)));
  store3(d.normal, normalize3(mul_n(N, V3(s.normal))));
  store3(d.tangent, normalize3(mul_n(N, V3(s.tangent))));
  d.tangent[3] = s.tangent[3];
  store3(bt, normalize3(mul_n(N, cross3(V3(s.normal), V3(s.tangent)) * s.tangent[3])));
  d.texcoord[0] = s.texcoord[0]; d.texcoord[1] = s.texcoord[1];
  return d;
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------------------------------
struct Box { float lo[3], hi[3]; };
PT_HD Box empty_box() {
  Box b;
  for (int k = 0; k < 3; ++k) { b.lo[k] = __builtin_inff(); b.hi[k] = -__builtin_inff(); }
  return b;
}
PT_HD void grow(Box& b, const float lo[3], const float hi[3]) {
  for (int k = 0; k < 3; ++k) { b.lo[k] = lo[k] < b.lo[k] ? lo[k] : b.lo[k]; b.hi[k] = hi[k] > b.hi[k] ? hi[k] : b.hi[k]; }
}
PT_HD void grow(Box& b, const Box& o) { grow(b, o.lo, o.hi); }
// a triangle's box: < and > from +-inf over the vertices in order
PT_HD Box triangle_box(const float a[3], const float b[3], const float c[3]) {
  Box t = empty_box();
  grow(t, a, a); grow(t, b, b); grow(t, c, c);
  return t;
}
PT_HD float half_area(const float lo[3], const float hi[3]) {
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  return ex * ey + ey * ez + ez * ex;
}
PT_HD float half_area(const Box& b) { return half_area(b.lo, b.hi); }
PT_HD float centre(const Box& b, int k) { return 0.5f * (b.lo[k] + b.hi[k]); }
// order-preserving map float <-> uint32 (negative values below positive ones): what integer atomic min / max take
PT_HD uint32_t ordered_u(float f) { const uint32_t u = __builtin_bit_cast(uint32_t, f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
PT_HD float unordered_f(uint32_t enc) { return __builtin_bit_cast(float, (enc & 0x80000000u) ? (enc ^ 0x80000000u) : ~enc); }

// ---- records ----------------------------------------------------------------------------------------------------------------------------------------
// triangle record, 3 units: (v0, primitive id) (e1, material class) (e2, 0)
PT_HD void tri_record(float4* o, const float a[3], const float b[3], const float c[3], uint32_t prim, uint32_t cls) {
  o[0] = make_float4(a[0], a[1], a[2], __builtin_bit_cast(float, prim));
  o[1] = make_float4(b[0] - a[0], b[1] - a[1], b[2] - a[2], __builtin_bit_cast(float, cls));
  o[2] = make_float4(c[0] - a[0], c[1] - a[1], c[2] - a[2], 0.0f);
}
// shading record: positions and normals of the three vertices, material and emitter index (5 units); tex: also uv, tangent and bitangent (units 5..10 of 12)
PT_HD void shading_record(float4* o, bool tex, const HostVertex& a, const HostVertex& b, const HostVertex& c, const float* ba, const float* bb, const float* bc,
                          int32_t material, int32_t emitter) {
  o[0] = make_float4(a.position[0], a.position[1], a.position[2], __builtin_bit_cast(float, material));
  o[1] = make_float4(b.position[0], b.position[1], b.position[2], __builtin_bit_cast(float, emitter));
  o[2] = make_float4(c.position[0], c.position[1], c.position[2], a.normal[0]);
  o[3] = make_float4(a.normal[1], a.normal[2], b.normal[0], b.normal[1]);
  o[4] = make_float4(b.normal[2], c.normal[0], c.normal[1], c.normal[2]);
  if (tex) {
    o[5] = make_float4(a.texcoord[0], a.texcoord[1], b.texcoord[0], b.texcoord[1]);
    o[6] = make_float4(c.texcoord[0], c.texcoord[1], a.tangent[0], a.tangent[1]);
    o[7] = make_float4(a.tangent[2], b.tangent[0], b.tangent[1], b.tangent[2]);
    o[8] = make_float4(c.tangent[0], c.tangent[1], c.tangent[2], ba[0]);
    o[9] = make_float4(ba[1], ba[2], bb[0], bb[1]);
    o[10] = make_float4(bb[2], bc[0], bc[1], bc[2]);
  }
}

// ---- Morton codes and surface-area bins: both cut the bounds cl..ch of the box centres into equal cells ----------------------------------------------
PT_HD float cell_scale(float cl, float ch, float cells) { return ch > cl ? cells / (ch - cl) : 0.0f; }      // 0 on a degenerate axis
PT_HD uint64_t spread21(uint32_t v) {       // bit i of v -> bit 3 i
  uint64_t x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
// Morton code, 63 bits: per axis 2^21 cells (scale = cell_scale(cl, ch, kMortonCells)) spread to every third bit; the caller shifts y by 1 and z by 2
constexpr float kMortonCells = 2097152.0f;
PT_HD uint64_t morton_axis(float c, float cl, float scale) {
  const float f = (c - cl) * scale;
  return spread21(f >= kMortonCells - 1.0f ? (uint32_t)kMortonCells - 1u : (uint32_t)f);
}
// the bin of a centre c >= cl (cl is the minimum of the centres binned): the last cell is clamped, c == ch lands in it
PT_HD int sah_bin(float c, float cl, float scale) {
  const int j = (int)((c - cl) * scale);
  return j > kSahBins - 1 ? kSahBins - 1 : j;
}
PT_HD float sah_suffix_area(const Box& suffix, uint32_t count) { return count ? half_area(suffix) : 0.0f; }
// cost of cutting behind a bin: half_area(L)·nL + half_area(R)·nR
PT_HD float sah_cut_cost(const Box& prefix, uint32_t prefix_count, float suffix_area, uint32_t suffix_count) {
  return half_area(prefix) * (float)prefix_count + suffix_area * (float)suffix_count;
}

// ---- 8-wide collapse (Ylitie, Karras, Laine 2017, sec. 3.1): the cost table of a binary node ----------------------------------------------------------
// C(n, i) = least cost of representing n's subtree by at most i roots.  c[i - 1] = C(n, i), i = 1..7; bits: 0 leaf1, i (2..7) same[i]: C(n, i) = C(n, i - 1),
// 8 + 3 (j - 2) ..: k[j], j = 2..8, the roots the left child gets of j.  Ties: leaf over interior, fewer roots over more, smallest k.
struct DpT { uint32_t bits; float c[7]; };
PT_HD int min7(int k) { return k > 7 ? 7 : k; }
PT_HD bool dp_leaf1(uint32_t bits) { return (bits & 1u) != 0u; }
PT_HD int dp_k(uint32_t bits, int j) { return (int)((bits >> (8 + 3 * (j - 2))) & 7u); }
// cost rows row[1..7] of a child link: a single triangle costs its test whatever the number of roots
PT_HD void dp_row(float area_of_triangle, float row[8]) { const float a = area_of_triangle * 1.0f * kCostPrim; for (int i = 1; i <= 7; ++i) row[i] = a; }
PT_HD void dp_row(const DpT& d, float row[8]) { for (int i = 1; i <= 7; ++i) row[i] = d.c[i - 1]; }
// C_dist(n, j) = min_k C(left, k) + C(right, j - k) for j = 2..8 from the children's rows; returns the k[j] bits of the table
PT_HD uint32_t collapse_dist(const float cl[8], const float cr[8], float dist[9]) {
  uint32_t bits = 0u;
  for (int j = 2; j <= 8; ++j) {
    float best = __builtin_inff(); int bk = 1;
    for (int k = 1; k < j; ++k) {
      const float v = cl[min7(k)] + cr[min7(j - k)];
      if (v < best) { best = v; bk = k; }
    }
    dist[j] = best; bits |= (uint32_t)bk << (8 + 3 * (j - 2));
  }
  return bits;
}
// the table from C_dist, the triangles below the node and the half area of its box
PT_HD DpT collapse_table(uint32_t kbits, const float dist[9], uint32_t tris, float area) {
  DpT d;
  d.bits = kbits;
  const float cleaf = tris <= (uint32_t)kLeafMax ? area * (float)tris * kCostPrim : __builtin_inff();
  const float cint = dist[8] + area * kCostNode;
  const bool leaf1 = cleaf <= cint;
  if (leaf1) d.bits |= 1u;
  d.c[0] = leaf1 ? cleaf : cint;
  for (int i = 2; i <= 7; ++i) {
    if (dist[i] < d.c[i - 2]) d.c[i - 1] = dist[i]; else { d.c[i - 1] = d.c[i - 2]; d.bits |= 1u << i; }
  }
  return d;
}
// One step of "the best forest of at most i roots below a node": false: the node itself is a root; true: its left child gets il roots, its right child ir
PT_HD bool forest_split(uint32_t bits, int i, int& il, int& ir) {
  while (i > 1 && ((bits >> i) & 1u)) --i;
  if (i == 1) return false;
  const int kk = dp_k(bits, i);
  il = min7(kk); ir = min7(i - kk);
  return true;
}
// slot_of[i]: child i of n goes where it lies in the node — slot s = octant s (bit k of s set = towards +axis k): repeatedly the (child, free slot) pair with
// the largest +-dx +-dy +-dz, d = child centre - node centre; ties to the lowest child, then the lowest slot
template <class Child> PT_HD void assign_slots(const Child* kid, int n, int* slot_of) {      // Child: anything with a Box `box`
  Box nb = empty_box();
  for (int i = 0; i < n; ++i) grow(nb, kid[i].box);
  float d[kWide][3];
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) d[i][k] = centre(kid[i].box, k) - centre(nb, k);
  uint32_t child_done = 0, slot_used = 0;
  for (int round = 0; round < n; ++round) {
    int bi = -1, bs = -1; float bsc = 0.0f;
    for (int i = 0; i < n; ++i) {
      if ((child_done >> i) & 1u) continue;
      for (int sl = 0; sl < kWide; ++sl) {
        if ((slot_used >> sl) & 1u) continue;
        const float sc = ((sl & 1) ? d[i][0] : -d[i][0]) + ((sl & 2) ? d[i][1] : -d[i][1]) + ((sl & 4) ? d[i][2] : -d[i][2]);
        if (bi < 0 || sc > bsc) { bi = i; bs = sl; bsc = sc; }
      }
    }
    child_done |= 1u << bi; slot_used |= 1u << bs; slot_of[bi] = bs;
  }
}

// ---- layout: the link of a leaf slot, the units of a children block (nodes of 4 units, then triangles of 3, padded to 64 bytes) -----------------------
PT_HD uint32_t leaf_code(uint32_t first, uint32_t count) { return ~(first | ((count - 1u) << 28)); }
PT_HD uint32_t block_units(uint32_t interior, uint32_t triangles) { return (4u * interior + 3u * triangles + 3u) & ~3u; }

// ---- the node record: origin on the 16-bit scene grid, 8-bit child planes at a power-of-two scale -----------------------------------------------------
PT_HD float grid_point(uint32_t q, float lo, float step) { return pt_fma((float)q, step, lo); }
// rounded down: the largest q with grid_point(q) <= the node's lower bound
PT_HD uint32_t grid_origin(float nlo, float lo, float step) {
  float fq = __builtin_floorf((nlo - lo) / step);
  if (fq < 0.0f) fq = 0.0f;
  if (fq > kGridCells) fq = kGridCells;
  uint32_t q16 = (uint32_t)fq;
  while (q16 > 0u && grid_point(q16, lo, step) > nlo) --q16;
  return q16;
}
// the first biased exponent to try: the smallest power of two >= (nhi - org) / 255, at least 2^-126
PT_HD uint32_t first_plane_exponent(float nhi, float org) {
  const uint32_t u = __builtin_bit_cast(uint32_t, (nhi - org) / 255.0f);
  uint32_t e = (u >> 23) & 255u;
  if (u & 0x007fffffu) e += 1u;
  return e < 1u ? 1u : e;
}
// one child's [lo, hi] on one axis at scale 2^(e - 127): the lower plane floored, the upper ceiled, each nudged until org + q·scale brackets the exact plane.
// fits == false: the upper plane lies beyond 255 cells — the caller goes on to the next exponent (ql, qh are clamped then, and nobody keeps them)
struct Planes { uint32_t ql, qh; bool fits; };
PT_HD Planes quantize_planes(float lo, float hi, float org, uint32_t e) {
  Planes r;
  r.fits = true;
  const float sc = __builtin_bit_cast(float, e << 23);
  float fl = __builtin_floorf((lo - org) / sc);
  if (fl < 0.0f) fl = 0.0f;
  if (fl > 255.0f) fl = 255.0f;
  int q = (int)fl;
  while (q > 0 && org + (float)q * sc > lo) --q;
  r.ql = (uint32_t)q;
  float ce = __builtin_ceilf((hi - org) / sc);
  if (ce < 0.0f) ce = 0.0f;
  if (ce > 255.0f) { r.fits = false; ce = 255.0f; }
  int q2 = (int)ce;
  while (q2 < 255 && org + (float)q2 * sc < hi) ++q2;
  if (org + (float)q2 * sc < hi) r.fits = false;
  r.qh = (uint32_t)q2;
  return r;
}
PT_HD uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }
// words 0..2 of a node: w0 oq.x | oq.y<<16   w1 oq.z | ex<<16 | ey<<24   w2 ez | imask<<8 | lmask<<16 | two<<24   (word 3 is its children block).
// The three slot masks are the tree's topology: a refit takes them from the word 2 it rewrites (node_masks_of), a build from the slots (node_masks).
PT_HD uint32_t node_masks(uint32_t imask, uint32_t lmask, uint32_t two) { return (imask << 8) | (lmask << 16) | (two << 24); }
PT_HD uint32_t node_masks_of(uint32_t word2) { return word2 & 0xffffff00u; }
PT_HD void node_header(const uint32_t oq[3], const uint32_t e[3], uint32_t masks, uint32_t w[3]) {
  w[0] = oq[0] | (oq[1] << 16);
  w[1] = oq[2] | (e[0] << 16) | (e[1] << 24);
  w[2] = e[2] | masks;
}
// one child slot's term of ptc_stats.bvh_sa_cost: half_area(child) / half_area(scene box when the topology was made), a two-triangle leaf twice, truncated to
// 2^-20 — summed as integers, so the sum is the same in any order
PT_HD uint64_t sa_cost_term(const Box& child, float scene_area, bool two_triangles) {
  const uint64_t term = (uint64_t)((half_area(child) / scene_area) * PTC_SA_COST_ONE);
  return two_triangles ? 2u * term : term;
}
}  // namespace scene_rules
