// The host side of the shared arithmetic (csrc/pt_device.h through pt_lens.h, pt_probes.h, pt_lights.h, pt_display.h, and pt_scene_rules.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU, no library.  It calls pt_lens_ray (pinhole, disk, 5 blades), pt_probe_dir, pt_light_sample (point,
// spot, directional) and pt_display_host_pixel8 (every operator x transfer function) on a few hundred inputs, special values among them, then the scene-build
// rules at their edges (a flat node, children that need the plane nudges, grid cells 0 and 65535, degenerate Morton / SAH axes, a collapse table over two
// single triangles, the records, the slots), and prints a checksum.
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Iphysically-based-renderer_amd/csrc tools/host_arithmetic_san.cpp -o /tmp/host_arithmetic_san && /tmp/host_arithmetic_san
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "pt_lens.h"
#include "pt_probes.h"
#include "pt_lights.h"
#include "pt_display.h"
#include "pt_scene_rules.h"
using namespace scene_rules;

int main() {
  uint64_t sum = 0;
  auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; ++i) sum = sum * 1099511628211ull + ((const unsigned char*)p)[i]; };
  const uint32_t sh = seed_hash(0x123456789abcdef0ull);
  DevCamera cam{};
  cam.pos[0] = 0.5f; cam.pos[1] = 1.0f; cam.pos[2] = 4.0f;
  cam.s[0] = 1.0f; cam.u[1] = -1.0f; cam.f[2] = -1.0f; cam.sx = 0.7f; cam.sy = 0.4f;
  const int w = 37, h = 23;
  for (int variant = 0; variant < 3; ++variant) {
    ptc_lens_params L{};
    L.aperture_radius = variant ? 0.05f : 0.0f; L.focus_distance = 3.0f; L.blades = variant == 2 ? 5 : 0; L.rotation = 0.13f;
    for (uint32_t i = 0; i < 400; ++i) {
      float o[3], d[3]; uint32_t key;
      pt_lens_ray(cam, L, w, h, sh, (i * 7919u) % (uint32_t)(w * h), i % 5u, o, d, key);
      mix(o, sizeof o); mix(d, sizeof d); mix(&key, sizeof key);
    }
  }
  for (uint32_t i = 0; i < 400; ++i) {
    float d[3]; uint32_t key;
    pt_probe_dir(sh, 0xfffffff0u + i, i * 3u, d, key);
    mix(d, sizeof d); mix(&key, sizeof key);
    float shc[PT_SH9_FLOATS], out[3];
    for (int k = 0; k < PT_SH9_FLOATS; ++k) shc[k] = pt_sh9_basis(k % PT_SH9, d[0], d[1], d[2]) * pt_sh9_resolve_scale(i + 1u);
    pt_sh9_eval(shc, d, out); mix(out, sizeof out);
    pt_sh9_irradiance(shc, d, out); mix(out, sizeof out);
  }
  const int types[3] = {PTC_LIGHT_POINT, PTC_LIGHT_SPOT, PTC_LIGHT_DIRECTIONAL};
  for (int t = 0; t < 3; ++t) {
    ptc_light_params p{};
    p.type = types[t]; p.position[0] = 1.0f; p.position[1] = 2.0f; p.position[2] = -0.5f;
    p.direction[0] = 0.3f; p.direction[1] = -1.0f; p.direction[2] = 0.2f;
    p.intensity[0] = 60.0f; p.intensity[1] = 55.0f; p.intensity[2] = 45.0f;
    p.range = t == 1 ? 0.0f : 6.0f; p.cos_inner = 0.9f; p.cos_outer = 0.7f; p.sampling_weight = 1.0f;
    if (pt_light_params_error(p)) { std::printf("light parameters rejected: %s\n", pt_light_params_error(p)); return 1; }
    pt_light_normalise(p);
    std::vector<ptc_light_params> one(1, p); std::vector<pt_light_rec> recs; std::vector<float> cdf;
    pt_light_table(one, recs, cdf);
    for (uint32_t i = 0; i < 300; ++i) {
      const v3 P = i == 0 ? V3(p.position) : V3(rng_f(i, 0, 0) * 8.0f - 4.0f, rng_f(i, 0, 1) * 8.0f - 4.0f, rng_f(i, 0, 2) * 8.0f - 4.0f);      // i = 0: P on the light
      v3 wi = V3(0, 0, 0), Li = V3(0, 0, 0); float dist = 0.0f;
      const bool ok = pt_light_sample(recs[0], P, wi, dist, Li);
      mix(&ok, sizeof ok); mix(&wi, sizeof wi); mix(&Li, sizeof Li); mix(&dist, sizeof dist);
    }
  }
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float special[] = {0.0f, -0.0f, 1e-30f, 0.08f, 0.76f, 0.0031308f, 1.0f, 4.0f, 1e6f, 3.0e38f, -1.0f, inf, -inf, nan};
  ptc_display_params dp; pt_display_defaults(dp);
  for (int op = PTC_TONEMAP_ACES; op <= PTC_TONEMAP_CLAMP; ++op)
    for (int oetf : {PTC_OETF_GAMMA22, PTC_OETF_SRGB}) {
      dp.tonemap = op; dp.oetf = oetf;
      if (pt_display_params_error(dp)) { std::printf("display parameters rejected\n"); return 1; }
      for (uint32_t i = 0; i < 300; ++i) {
        float c[4] = {rng_f(i, 1, 0) * 20.0f - 0.1f, rng_f(i, 1, 1) * 20.0f - 0.1f, rng_f(i, 1, 2) * 20.0f - 0.1f, rng_f(i, 1, 3) * 1.2f - 0.1f};
        if (i < 14u * 4u) c[i % 4u] = special[i / 4u];
        const uint32_t v = pt_display_host_pixel8(dp, i % 3u ? 3.7f : 1.0f, c);
        uint32_t lo, hi; pt_display_pixel16(c[0], c[1], c[2], c[3], 3.7f, lo, hi);
        mix(&v, sizeof v); mix(&lo, sizeof lo); mix(&hi, sizeof hi);
      }
    }
  // ---- pt_scene_rules.h ----
  {
    HostVertex sv{};
    sv.position[0] = 1.0f; sv.position[1] = -2.0f; sv.position[2] = 0.5f; sv.normal[1] = 1.0f; sv.tangent[0] = 1.0f; sv.tangent[3] = -1.0f; sv.texcoord[0] = 0.25f;
    const float m16[16] = {2, 0, 0, 0, 0, 0, 3, 0, 0, -1, 0, 0, 5, 6, 7, 1}, n9[9] = {0.5f, 0, 0, 0, 0, -1.0f, 0, 1.0f / 3.0f, 0};
    float m12[12], bt[3][3];
    for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) m12[c * 3 + r] = m16[c * 4 + r];
    HostVertex w[3];
    w[0] = world_vertex(m16, 4, n9, sv, bt[0]);
    w[1] = world_vertex(m12, 3, n9, sv, bt[1]);
    if (std::memcmp(&w[0], &w[1], sizeof w[0]) != 0) { std::printf("world_vertex: column stride 4 and 3 differ\n"); return 1; }
    sv.position[0] = 4.0f; w[1] = world_vertex(m16, 4, n9, sv, bt[1]);
    sv.position[2] = -3.0f; w[2] = world_vertex(m16, 4, n9, sv, bt[2]);
    mix(w, sizeof w); mix(bt, sizeof bt);
    const Box tb = triangle_box(w[0].position, w[1].position, w[2].position);
    mix(&tb, sizeof tb);
    std::vector<float4> rec(3 + 12);
    tri_record(rec.data(), w[0].position, w[1].position, w[2].position, 7u, 3u);
    shading_record(rec.data() + 3, true, w[0], w[1], w[2], bt[0], bt[1], bt[2], 5, -1);
    mix(rec.data(), 14 * sizeof(float4));
    std::vector<float4> rec5(5);      // an untextured record ends after 5 units: one more would be a heap overflow
    shading_record(rec5.data(), false, w[0], w[1], w[2], bt[0], bt[1], bt[2], 5, -1);
    mix(rec5.data(), 5 * sizeof(float4));
    // grid: cell 0, cell 65535, below and beyond the box, a degenerate box (step 1)
    const float glo = -3.0f, ghi = 9.0f, step = (ghi - glo) / kGridCells;
    const float probes[] = {glo, ghi, glo - 1.0f, ghi + 1.0f, glo + step * 0.5f, grid_point(65535u, glo, step), grid_point(65534u, glo, step), 0.1f};
    for (float x : probes) {
      const uint32_t q = grid_origin(x, glo, step);
      if (q > 65535u || (q > 0u && grid_point(q, glo, step) > x)) { std::printf("grid_origin(%g) = %u is not rounded down\n", (double)x, q); return 1; }
      mix(&q, sizeof q);
    }
    if (grid_origin(glo, glo, step) != 0u || grid_origin(ghi + 1.0f, glo, step) != 65535u || grid_origin(2.0f, 2.0f, 1.0f) != 0u) { std::printf("grid_origin: edge cells\n"); return 1; }
    // planes: a flat node (nhi == org: the exponent clamps to 1), then children against origins far from zero, where org + q * scale rounds and the nudges run
    if (first_plane_exponent(2.5f, 2.5f) != 1u) { std::printf("first_plane_exponent: a flat node\n"); return 1; }
    { const Planes q = quantize_planes(2.5f, 2.5f, 2.5f, 1u); if (!q.fits || q.ql != 0u || q.qh != 0u) { std::printf("quantize_planes: a flat node\n"); return 1; } mix(&q, sizeof q); }
    uint32_t nudged = 0, refused = 0;
    for (uint32_t i = 0; i < 4000; ++i) {
      // odd i: the origin far below planes near zero, so that lo - org is rounded and the floored / ceiled cell can lie on the wrong side
      const float org = (i & 1u) ? -1000.0f - rng_f(i, 2, 0) : rng_f(i, 2, 0) * 1e-3f, ext = (i & 1u) ? 1000.0f + 500.0f * rng_f(i, 2, 1) : rng_f(i, 2, 1) * ((i & 2u) ? 50.0f : 1e-3f);
      const float nhi = org + ext, lo = (i & 1u) ? rng_f(i, 2, 2) * 1e-2f - 5e-3f : org + ext * rng_f(i, 2, 2), hi = lo + (nhi - lo) * rng_f(i, 2, 3) * ((i & 5u) == 5u ? 1e-6f : 1.0f);
      uint32_t e = first_plane_exponent(nhi, org);
      Planes q = quantize_planes(lo, hi, org, e);
      for (; !q.fits && e < 254u; ++refused) q = quantize_planes(lo, hi, org, ++e);
      const float sc = __builtin_bit_cast(float, e << 23);
      if (!q.fits || q.ql > 255u || q.qh > 255u || org + (float)q.ql * sc > lo || org + (float)q.qh * sc < hi) { std::printf("quantize_planes: child %u is not bracketed\n", i); return 1; }
      if ((q.ql > 0u && (float)q.ql != __builtin_floorf((lo - org) / sc)) || (float)q.qh != __builtin_ceilf((hi - org) / sc)) ++nudged;
      mix(&q, sizeof q); mix(&e, sizeof e);
    }
    // the nudges themselves: origin -1000, scale 4 (the node reaches 10), a child [-1e-10, 1e-10] around a plane of the grid: lo - org and hi - org both round to
    // 1000, so floor and ceil both say cell 250, whose plane is 0 — above lo and below hi; the loops move them to 249 and 251
    {
      const uint32_t e = first_plane_exponent(10.0f, -1000.0f);
      const Planes q = quantize_planes(-1e-10f, 1e-10f, -1000.0f, e);
      if (e != 129u || !q.fits || q.ql != 249u || q.qh != 251u) { std::printf("quantize_planes: the nudges (e %u ql %u qh %u)\n", e, q.ql, q.qh); return 1; }
      const Planes top = quantize_planes(-1e-10f, 20.001f, -1000.0f, e);      // an upper plane one cell beyond 255 does not fit
      if (top.fits) { std::printf("quantize_planes: the upper plane beyond 255 cells\n"); return 1; }
      mix(&q, sizeof q); mix(&top, sizeof top);
    }
    // Morton and SAH cells: a degenerate axis has scale 0 and everything in cell 0; the last cell is clamped
    if (cell_scale(1.5f, 1.5f, kMortonCells) != 0.0f || morton_axis(1.5f, 1.5f, 0.0f) != 0u || sah_bin(1.5f, 1.5f, 0.0f) != 0) { std::printf("degenerate axis\n"); return 1; }
    if (morton_axis(2.0f, 1.0f, cell_scale(1.0f, 2.0f, kMortonCells)) != spread21(2097151u) || sah_bin(2.0f, 1.0f, cell_scale(1.0f, 2.0f, (float)kSahBins)) != kSahBins - 1) { std::printf("last cell\n"); return 1; }
    for (uint32_t i = 0; i < 300; ++i) {
      const float c = rng_f(i, 3, 0) * 7.0f - 2.0f;
      const uint64_t code = morton_axis(c, -2.0f, cell_scale(-2.0f, 5.0f, kMortonCells)) << (i % 3u);
      const int j = sah_bin(c, -2.0f, cell_scale(-2.0f, 5.0f, (float)kSahBins));
      const uint32_t o = ordered_u(c);
      if (unordered_f(o) != c || j < 0 || j >= kSahBins) { std::printf("cells\n"); return 1; }
      mix(&code, sizeof code); mix(&j, sizeof j); mix(&o, sizeof o);
    }
    const float cost = sah_cut_cost(tb, 3u, sah_suffix_area(tb, 0u), 0u) + sah_cut_cost(empty_box(), 0u, sah_suffix_area(tb, 2u), 2u);      // an empty side: inf - inf is a NaN that nobody compares
    mix(&cost, sizeof cost);
    // collapse: two single triangles under one node (a leaf of two), then that table under a node of three
    float cl[8], cr[8], dist[9];
    dp_row(half_area(tb), cl); dp_row(2.0f, cr);
    const DpT two = collapse_table(collapse_dist(cl, cr, dist), dist, 2u, 10.0f);
    dp_row(two, cl);
    const DpT three = collapse_table(collapse_dist(cl, cr, dist), dist, 3u, 20.0f);
    int il = 0, ir = 0;
    if (!dp_leaf1(two.bits) || dp_leaf1(three.bits) || forest_split(two.bits, 7, il, ir) || !forest_split(three.bits, 7, il, ir) || il + ir < 2 || dp_k(three.bits, 8) < 1) { std::printf("collapse tables\n"); return 1; }
    mix(&two, sizeof two); mix(&three, sizeof three);
    // slots: 1, 2 and 8 children, coincident boxes among them
    struct { int id; Box box; } kids[kWide];
    for (int i = 0; i < kWide; ++i) { kids[i].id = i; kids[i].box = tb; for (int k = 0; k < 3; ++k) { kids[i].box.lo[k] += (float)((i >> k) & 1); kids[i].box.hi[k] += (float)((i >> k) & 1); } }
    kids[5] = kids[2];
    for (int n : {1, 2, kWide}) {
      int slot_of[kWide]; uint32_t used = 0;
      assign_slots(kids, n, slot_of);
      for (int i = 0; i < n; ++i) { if (slot_of[i] < 0 || slot_of[i] >= kWide || ((used >> slot_of[i]) & 1u)) { std::printf("assign_slots\n"); return 1; } used |= 1u << slot_of[i]; }
      mix(slot_of, n * sizeof(int));
    }
    uint32_t w3[3]; const uint32_t oq[3] = {0u, 65535u, 1u}, e3[3] = {1u, 254u, 127u};
    node_header(oq, e3, node_masks(0x81u, 0x7eu, 0x42u), w3);
    if (node_masks_of(w3[2]) != node_masks(0x81u, 0x7eu, 0x42u) || pack4(255u, 0u, 1u, 254u) != 0xfe0100ffu) { std::printf("node header\n"); return 1; }
    const uint64_t term = sa_cost_term(tb, half_area(tb), true) + sa_cost_term(kids[7].box, half_area(tb), false);
    const uint32_t lc = leaf_code((1u << 28) - 1u, 2u), bu = block_units(8u, 0u) + block_units(0u, 16u) + block_units(1u, 1u);
    mix(w3, sizeof w3); mix(&term, sizeof term); mix(&lc, sizeof lc); mix(&bu, sizeof bu);
    std::printf("scene rules: 4000 random children bracketed (%u nudged, %u exponents refused), the constructed nudges and edges as expected\n", nudged, refused);
  }
  std::printf("host arithmetic: checksum %016llx\n", (unsigned long long)sum);
  return 0;
}
