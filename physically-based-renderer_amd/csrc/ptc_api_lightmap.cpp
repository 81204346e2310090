// ptc_api_lightmap.cpp — lightmaps over the C-ABI (pt_lightmap.h, include/ptc_lightmap.h): the texel list of an instance's atlas, the lightmap frame
// (frame_begin's entry branch and run_batch do the rest), the resolve into the atlas with validity and dilation, and the ptc_debug_lightmap_* hooks.
#include "ptc_ctx.h"

#include <cmath>

using namespace ptc_detail;

namespace {
// What a description says about the instance to bake: its slice of the committed scene's world vertices and primitives, and the atlas UVs of its vertices
struct LmSource { uint32_t vert_first = 0, tri_first = 0, n_verts = 0, n_tris = 0; std::vector<float> uv; };

// PTC_E_ARG for what the header lists (with_budget: spp_total and max_bounces are read), nothing changed; else the source
int lm_check(ptc_ctx* c, const ptc_lightmap_desc* d, const std::string& who, bool with_budget, LmSource& src) {
  if (!d) return fail(c, PTC_E_ARG, who + ": null pointer");
  if (d->instance < 0 || (size_t)d->instance >= c->insts.size()) return fail(c, PTC_E_ARG, who + ": unknown instance");
  if (d->width < 1 || d->width > PT_LM_MAX_SIDE || d->height < 1 || d->height > PT_LM_MAX_SIDE) return fail(c, PTC_E_ARG, who + ": width or height outside 1..8192");
  if (with_budget && (d->spp_total < 1 || d->max_bounces < 0)) return fail(c, PTC_E_ARG, who + ": spp_total < 1 or max_bounces < 0");
  if ((uint64_t)d->texel_index_base + (uint64_t)d->width * (uint64_t)d->height > 0x100000000ull) return fail(c, PTC_E_ARG, who + ": texel indices exceed 32 bits");
  for (int i = 0; i < d->instance; ++i) {
    const HostMesh& m = c->meshes[(size_t)c->insts[(size_t)i].mesh];
    src.vert_first += (uint32_t)m.v.size(); src.tri_first += (uint32_t)(m.idx.size() / 3);
  }
  const HostMesh& m = c->meshes[(size_t)c->insts[(size_t)d->instance].mesh];
  src.n_verts = (uint32_t)m.v.size(); src.n_tris = (uint32_t)(m.idx.size() / 3);
  src.uv.resize((size_t)src.n_verts * 2);
  for (size_t i = 0; i < src.n_verts; ++i)
    for (int k = 0; k < 2; ++k) {
      const float u = d->uv ? d->uv[i * 2 + (size_t)k] : m.v[i].texcoord[k];
      if (!std::isfinite(u)) return fail(c, PTC_E_ARG, who + ": a uv is not finite");
      src.uv[i * 2 + (size_t)k] = u;
    }
  return PTC_OK;
}
int lm_committed(ptc_ctx* c, const std::string& who) {
  if (!c->committed) return fail(c, PTC_E_STATE, who + ": scene not committed");
  if (!description_matches_commit(c)) return fail(c, PTC_E_STATE, who + ": the scene's meshes or instances changed since the commit");
  return PTC_OK;
}

// ---- the host evaluation of pt_lightmap.h (a description-only context) ---------------------------------------------------------------------------------
pt_lm_tri lm_host_tri(const DevLmGeom& g, uint32_t tri, uint32_t i[3]) {
  for (int k = 0; k < 3; ++k) i[k] = g.widx[(size_t)tri * 3 + (size_t)k] - g.vert_first;
  return pt_lm_make_tri(g.uv + (size_t)i[0] * 2, g.uv + (size_t)i[1] * 2, g.uv + (size_t)i[2] * 2, g.w, g.h);
}
void lm_host_cover(const DevLmGeom& g, std::vector<uint32_t>& owner) {
  owner.assign((size_t)g.w * (size_t)g.h, PT_LM_NONE);
  for (uint32_t tri = 0; tri < g.n_tris; ++tri) {
    uint32_t i[3];
    const pt_lm_tri t = lm_host_tri(g, tri, i);
    int x0, x1, y0, y1;
    pt_lm_box(t, g.w, g.h, x0, x1, y0, y1);
    for (int y = y0; y <= y1; ++y)
      for (int x = x0; x <= x1; ++x) {
        int64_t e[3];
        uint32_t& o = owner[(size_t)y * (size_t)g.w + (size_t)x];
        if (pt_lm_edges(t, x, y, e) && tri < o) o = tri;
      }
  }
}
// the list in ascending atlas index: two float4 per entry as k_lm_texels writes them; returns the number of owned texels dropped
uint32_t lm_host_texels(const DevLmGeom& g, const std::vector<uint32_t>& owner, float ray_eps, std::vector<float4>& texels) {
  uint32_t dropped = 0;
  texels.clear();
  for (size_t a = 0; a < owner.size(); ++a) {
    const uint32_t tri = owner[a];
    if (tri == PT_LM_NONE) continue;
    uint32_t i[3];
    const pt_lm_tri t = lm_host_tri(g, tri, i);
    const v3 p0 = V3(g.verts[i[0]].position), p1 = V3(g.verts[i[1]].position), p2 = V3(g.verts[i[2]].position);
    if (!pt_lm_finite3(pt_lm_face_normal(p0, p1, p2))) { ++dropped; continue; }
    int64_t e[3];
    pt_lm_edges(t, (int)(a % (size_t)g.w), (int)(a / (size_t)g.w), e);
    v3 o, n;
    pt_lm_texel(e, p0, p1, p2, V3(g.verts[i[0]].normal), V3(g.verts[i[1]].normal), V3(g.verts[i[2]].normal), ray_eps, o, n);
    texels.push_back(make_float4(o.x, o.y, o.z, __builtin_bit_cast(float, (uint32_t)a)));
    texels.push_back(make_float4(n.x, n.y, n.z, __builtin_bit_cast(float, tri)));
  }
  return dropped;
}

// ---- the device side ---------------------------------------------------------------------------------------------------------------------------------
template <class T> int lm_upload(ptc_ctx* c, DevBuf<T>& b, const T* src, size_t n) {
  { int rc = ensure_buf(c, b, n); if (rc) return rc; }
  if (n) HIP_TRY(c, hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return PTC_OK;
}
// The instance's geometry for the kernels.  World vertices and indices come from HBM where the device made them last (a commit, refit or rebuild on the device left the
// host's copy stale), else from the host build: either way the transforms and poses of the last commit, refit or rebuild
int lm_device_geom(ptc_ctx* c, const LmSource& src, int w, int h, DevLmGeom& g) {
  Lightmap& L = c->lightmap;
  const CommittedScene& s = c->scene;
  { int rc = lm_upload(c, L.uv, src.uv.data(), src.uv.size()); if (rc) return rc; }
  g.uv = L.uv.p; g.vert_first = src.vert_first; g.n_tris = src.n_tris; g.w = w; g.h = h;
  if (s.host_stale && s.refit_ready) {
    g.verts = s.drf.wverts + src.vert_first; g.widx = s.drf.widx + (size_t)src.tri_first * 3;
    return PTC_OK;
  }
  const HostBuilt& B = *c->built;
  if (B.wverts.size() < (size_t)src.vert_first + src.n_verts || B.widx.size() < ((size_t)src.tri_first + src.n_tris) * 3) return fail(c, PTC_E_STATE, "lightmap: the host build holds no world vertices");
  { int rc = lm_upload(c, L.verts, B.wverts.data() + src.vert_first, (size_t)src.n_verts); if (rc) return rc; }
  { int rc = lm_upload(c, L.idx, B.widx.data() + (size_t)src.tri_first * 3, (size_t)src.n_tris * 3); if (rc) return rc; }
  g.verts = L.verts.p; g.widx = L.idx.p;
  return PTC_OK;
}
// owner image -> list -> texel records on lane 0 (every lane is idle); the counts come back, so the call waits
int lm_build_list(ptc_ctx* c, const DevLmGeom& g, float ray_eps) {
  Lightmap& L = c->lightmap;
  const size_t n_texels = (size_t)g.w * (size_t)g.h;
  int rc = ensure_buf(c, L.owner, n_texels);
  if (!rc) rc = ensure_buf(c, L.flags, n_texels);
  if (!rc) rc = ensure_buf(c, L.list, n_texels);
  if (!rc) rc = ensure_buf(c, L.block, (size_t)pt_lm_blocks((uint32_t)n_texels));
  if (!rc) rc = ensure_buf(c, L.counts, (size_t)2);
  if (rc) return rc;
  hipStream_t st = c->lanes[0].stream;
  pt_launch_lm_cover(st, g, L.owner.p);
  pt_launch_lm_list(st, g, L.owner.p, DevLmScratch{L.flags.p, L.block.p, L.counts.p}, L.list.p);
  HIP_TRY(c, hipGetLastError());
  uint32_t counts[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(counts, L.counts.p, sizeof counts, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (counts[0] > n_texels) return fail(c, PTC_E_DEVICE, "lightmap: the texel list is longer than the atlas");
  if ((rc = ensure_buf(c, L.texels, (size_t)counts[0] * 2))) return rc;
  pt_launch_lm_texels(st, g, L.owner.p, L.list.p, counts[0], ray_eps, L.texels.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));
  L.n = counts[0]; L.dropped = counts[1]; L.w = g.w; L.h = g.h;
  return PTC_OK;
}
// what a debug hook on a device context does first: idle lanes, the frame ended
int lm_debug_prepare(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  return PTC_OK;
}
void lm_split_texels(const float4* T, size_t n, uint32_t* atlas_index, uint32_t* prim, float* origin_xyz, float* normal_xyz) {
  for (size_t e = 0; e < n; ++e) {
    const float4 a = T[e * 2], b = T[e * 2 + 1];
    if (atlas_index) atlas_index[e] = __builtin_bit_cast(uint32_t, a.w);
    if (prim) prim[e] = __builtin_bit_cast(uint32_t, b.w);
    if (origin_xyz) { origin_xyz[e * 3] = a.x; origin_xyz[e * 3 + 1] = a.y; origin_xyz[e * 3 + 2] = a.z; }
    if (normal_xyz) { normal_xyz[e * 3] = b.x; normal_xyz[e * 3 + 1] = b.y; normal_xyz[e * 3 + 2] = b.z; }
  }
}
}  // namespace

extern "C" {
int ptc_lightmap_begin(ptc_ctx* c, const ptc_lightmap_desc* d) {
  if (!c) return PTC_E_ARG;
  LmSource src;
  { int rc = lm_check(c, d, "lightmap_begin", true, src); if (rc) return rc; }
  { int rc = lm_committed(c, "lightmap_begin"); if (rc) return rc; }
  if (const char* why = medium_conflict(c, PTC_INTEGRATOR_PATH)) { c->in_frame = false; return fail(c, PTC_E_STATE, why); }
  { int rd = need_device(c); if (rd) return rd; }
  c->in_frame = false; c->pending = 0; drop_guides(c);      // whatever happens below, the previous frame is over
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  DevLmGeom g{};
  { int rc = lm_device_geom(c, src, d->width, d->height, g); if (rc) return rc; }
  { int rc = lm_build_list(c, g, c->built->ray_eps); if (rc) return rc; }
  const FrameEntries fe{"lightmap_begin", nullptr, d->texel_index_base};
  return frame_begin(c, (int)c->lightmap.n, 1, d->spp_total, d->seed, d->max_bounces, PTC_INTEGRATOR_PATH, 0, 1, &fe);
}

int ptc_lightmap_texel_count(ptc_ctx* c, uint32_t* covered, uint32_t* dropped) {
  if (!c) return PTC_E_ARG;
  if (!c->in_frame || !c->lightmap.on) return fail(c, PTC_E_STATE, "lightmap_texel_count: no lightmap frame (ptc_lightmap_begin)");
  if (covered) *covered = c->lightmap.n;
  if (dropped) *dropped = c->lightmap.dropped;
  return PTC_OK;
}

int ptc_lightmap_read_texels(ptc_ctx* c, uint32_t* atlas_index, uint32_t* prim, float* origin_xyz, float* normal_xyz) {
  if (!c) return PTC_E_ARG;
  if (!c->in_frame || !c->lightmap.on) return fail(c, PTC_E_STATE, "lightmap_read_texels: no lightmap frame (ptc_lightmap_begin)");
  { int rd = need_device(c); if (rd) return rd; }
  const size_t n = c->lightmap.n;
  std::vector<float4> T(n * 2);
  if (n) HIP_TRY(c, hipMemcpy(T.data(), c->lightmap.texels.p, T.size() * sizeof(float4), hipMemcpyDeviceToHost));      // written before the frame began: nothing to wait for
  lm_split_texels(T.data(), n, atlas_index, prim, origin_xyz, normal_xyz);
  return PTC_OK;
}

int ptc_lightmap_read(ptc_ctx* c, int dilate_iters, float backface_threshold, float* out_rgba, float* out_backface) {
  if (!c) return PTC_E_ARG;
  if (!out_rgba) return fail(c, PTC_E_ARG, "lightmap_read: null pointer");
  if (dilate_iters < 0 || dilate_iters > PT_LM_MAX_DILATE) return fail(c, PTC_E_ARG, "lightmap_read: dilate_iters outside 0..64");
  if (!(backface_threshold >= 0.0f) || !std::isfinite(backface_threshold)) return fail(c, PTC_E_ARG, "lightmap_read: the back-face threshold must be finite and >= 0");
  if (!c->in_frame || !c->lightmap.on) return fail(c, PTC_E_STATE, "lightmap_read: no lightmap frame (ptc_lightmap_begin)");
  { int rd = need_device(c); if (rd) return rd; }
  { int rf = flush(c); if (rf) return rf; }
  { int rj = join_lanes_on_stream0(c); if (rj) return rj; }
  Lightmap& L = c->lightmap;
  const size_t n_texels = (size_t)L.w * (size_t)L.h;
  const uint32_t N = c->resolve_divisor ? c->resolve_divisor : c->samples_done;
  int rc = ensure_buf(c, L.atlas[0], n_texels);
  if (!rc && dilate_iters) rc = ensure_buf(c, L.atlas[1], n_texels);
  if (!rc && out_backface) rc = ensure_buf(c, L.fraction, (size_t)L.n);
  if (rc) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipMemsetAsync(L.atlas[0].p, 0, n_texels * sizeof(float4), s0));
  if (out_backface && L.n) HIP_TRY(c, hipMemsetAsync(L.fraction.p, 0, (size_t)L.n * sizeof(float), s0));      // no sample yet: zeros
  pt_launch_lm_scatter(s0, L.texels.p, L.n, c->accum.p, L.back.p, N, backface_threshold, L.atlas[0].p, out_backface ? L.fraction.p : nullptr);
  int cur = 0;
  for (int i = 0; i < dilate_iters; ++i) { pt_launch_lm_dilate(s0, L.atlas[cur].p, L.atlas[cur ^ 1].p, L.w, L.h); cur ^= 1; }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s0));
  HIP_TRY(c, hipMemcpy(out_rgba, L.atlas[cur].p, n_texels * sizeof(float4), hipMemcpyDeviceToHost));
  if (out_backface && L.n) HIP_TRY(c, hipMemcpy(out_backface, L.fraction.p, (size_t)L.n * sizeof(float), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_render_lightmap(ptc_ctx* c, const ptc_lightmap_desc* d, int dilate_iters, float backface_threshold, float* out_rgba) {
  if (!c) return PTC_E_ARG;
  if (!out_rgba) return fail(c, PTC_E_ARG, "render_lightmap: null pointer");
  if (dilate_iters < 0 || dilate_iters > PT_LM_MAX_DILATE) return fail(c, PTC_E_ARG, "render_lightmap: dilate_iters outside 0..64");
  if (!(backface_threshold >= 0.0f) || !std::isfinite(backface_threshold)) return fail(c, PTC_E_ARG, "render_lightmap: the back-face threshold must be finite and >= 0");
  int rc = ptc_lightmap_begin(c, d);
  if (rc) return rc;
  if ((rc = ptc_frame_add_samples(c, d->spp_total))) return rc;
  return ptc_lightmap_read(c, dilate_iters, backface_threshold, out_rgba, nullptr);
}

// ---- test hooks ----------------------------------------------------------------------------------------------------------------------------------------
int ptc_debug_lightmap_cover(ptc_ctx* c, const uint32_t* indices, uint32_t n_tris, const float* uv, uint32_t n_verts, int width, int height, uint32_t* out_owner) {
  if (!c) return PTC_E_ARG;
  if (!indices || !uv || !out_owner || n_tris == 0 || n_tris >= (1u << 28) || n_verts == 0 || width < 1 || width > PT_LM_MAX_SIDE || height < 1 || height > PT_LM_MAX_SIDE)
    return fail(c, PTC_E_ARG, "debug_lightmap_cover: bad argument");
  for (size_t i = 0; i < (size_t)n_tris * 3; ++i)
    if (indices[i] >= n_verts) return fail(c, PTC_E_ARG, "debug_lightmap_cover: a vertex index is out of range");
  for (size_t i = 0; i < (size_t)n_verts * 2; ++i)
    if (!std::isfinite(uv[i])) return fail(c, PTC_E_ARG, "debug_lightmap_cover: a uv is not finite");
  DevLmGeom g{};
  g.vert_first = 0; g.n_tris = n_tris; g.w = width; g.h = height;
  const size_t n_texels = (size_t)width * (size_t)height;
  if (c->device < 0) {      // the host evaluation of pt_lightmap.h
    g.widx = indices; g.uv = uv;
    std::vector<uint32_t> owner;
    lm_host_cover(g, owner);
    std::memcpy(out_owner, owner.data(), n_texels * sizeof(uint32_t));
    return PTC_OK;
  }
  { int rc = lm_debug_prepare(c); if (rc) return rc; }
  Lightmap& L = c->lightmap;
  int rc = lm_upload(c, L.uv, uv, (size_t)n_verts * 2);
  if (!rc) rc = lm_upload(c, L.idx, indices, (size_t)n_tris * 3);
  if (!rc) rc = ensure_buf(c, L.owner, n_texels);
  if (rc) return rc;
  g.widx = L.idx.p; g.uv = L.uv.p;
  hipStream_t st = c->lanes[0].stream;
  pt_launch_lm_cover(st, g, L.owner.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipMemcpy(out_owner, L.owner.p, n_texels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_debug_lightmap_rays(ptc_ctx* c, const ptc_lightmap_desc* d, uint32_t first_sample, uint32_t n_samples, uint32_t* out_counts, uint32_t* atlas_index, uint32_t* prim,
                            float* origin_xyz, float* normal_xyz, float* out_o_d, uint32_t* out_key) {
  if (!c) return PTC_E_ARG;
  if (!out_counts) return fail(c, PTC_E_ARG, "debug_lightmap_rays: null pointer");
  LmSource src;
  { int rc = lm_check(c, d, "debug_lightmap_rays", false, src); if (rc) return rc; }
  const uint64_t n_texels = (uint64_t)d->width * (uint64_t)d->height;
  if (n_samples == 0 || n_texels * (uint64_t)n_samples > 0x7fffffffull || (uint64_t)first_sample + n_samples > 0x100000000ull)
    return fail(c, PTC_E_ARG, "debug_lightmap_rays: bad sample range");
  { int rc = lm_committed(c, "debug_lightmap_rays"); if (rc) return rc; }
  const uint32_t sh = ::seed_hash(d->seed), base = d->texel_index_base;
  const bool rays = out_o_d || out_key;
  if (c->device < 0) {      // the host evaluation of pt_lightmap.h, on the host build
    const HostBuilt& B = *c->built;
    DevLmGeom g{};
    g.verts = B.wverts.data() + src.vert_first; g.widx = B.widx.data() + (size_t)src.tri_first * 3; g.vert_first = src.vert_first; g.uv = src.uv.data();
    g.n_tris = src.n_tris; g.w = d->width; g.h = d->height;
    std::vector<uint32_t> owner;
    std::vector<float4> T;
    lm_host_cover(g, owner);
    out_counts[1] = lm_host_texels(g, owner, B.ray_eps, T);
    const size_t n = T.size() / 2;
    out_counts[0] = (uint32_t)n;
    lm_split_texels(T.data(), n, atlas_index, prim, origin_xyz, normal_xyz);
    for (size_t p = 0; rays && p < n * n_samples; ++p) {
      const size_t e = p % n;
      float dir[3]; uint32_t key;
      pt_lm_dir(sh, base + __builtin_bit_cast(uint32_t, T[e * 2].w), first_sample + (uint32_t)(p / n), V3(T[e * 2 + 1].x, T[e * 2 + 1].y, T[e * 2 + 1].z), dir, key);
      if (out_o_d) { float* o = out_o_d + p * 6; o[0] = T[e * 2].x; o[1] = T[e * 2].y; o[2] = T[e * 2].z; o[3] = dir[0]; o[4] = dir[1]; o[5] = dir[2]; }
      if (out_key) out_key[p] = key;
    }
    return PTC_OK;
  }
  { int rc = lm_debug_prepare(c); if (rc) return rc; }
  DevLmGeom g{};
  { int rc = lm_device_geom(c, src, d->width, d->height, g); if (rc) return rc; }
  { int rc = lm_build_list(c, g, c->built->ray_eps); if (rc) return rc; }
  const Lightmap& L = c->lightmap;
  const size_t n = L.n;
  out_counts[0] = L.n; out_counts[1] = L.dropped;
  std::vector<float4> T(n * 2);
  if (n) HIP_TRY(c, hipMemcpy(T.data(), L.texels.p, T.size() * sizeof(float4), hipMemcpyDeviceToHost));
  lm_split_texels(T.data(), n, atlas_index, prim, origin_xyz, normal_xyz);
  if (!rays || !n) return PTC_OK;
  const uint32_t n_paths = (uint32_t)(n * n_samples);
  { int rc = ensure_lane_queues(c, n_paths); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  pt_launch_raygen_texel(ln.stream, L.texels.p, L.n, base, sh, batch_queues(c, 0, n_paths), first_sample, n_samples);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::vector<float4> A(n_paths), Bq(n_paths), Cq(n_paths);
  HIP_TRY(c, hipMemcpy(A.data(), ln.q.ray[0].A, (size_t)n_paths * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(Bq.data(), ln.q.ray[0].B, (size_t)n_paths * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(Cq.data(), ln.q.ray[0].C, (size_t)n_paths * sizeof(float4), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < n_paths; ++p) {
    if (out_o_d) { float* o = out_o_d + p * 6; o[0] = A[p].x; o[1] = A[p].y; o[2] = A[p].z; o[3] = A[p].w; o[4] = Bq[p].x; o[5] = Bq[p].y; }
    if (out_key) std::memcpy(&out_key[p], &Cq[p].w, 4);
  }
  return PTC_OK;
}

int ptc_debug_lightmap_dilate(ptc_ctx* c, int width, int height, int iters, float* rgba_inout) {
  if (!c) return PTC_E_ARG;
  if (!rgba_inout || width < 1 || width > PT_LM_MAX_SIDE || height < 1 || height > PT_LM_MAX_SIDE || iters < 0 || iters > PT_LM_MAX_DILATE)
    return fail(c, PTC_E_ARG, "debug_lightmap_dilate: bad argument");
  const size_t n_texels = (size_t)width * (size_t)height;
  if (c->device < 0) {      // the host evaluation of pt_lightmap.h
    std::vector<float4> a(n_texels), b(n_texels);
    std::memcpy(a.data(), rgba_inout, n_texels * sizeof(float4));
    for (int i = 0; i < iters; ++i) {
      for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) b[(size_t)y * (size_t)width + (size_t)x] = pt_lm_dilate(a.data(), width, height, x, y);
      a.swap(b);
    }
    std::memcpy(rgba_inout, a.data(), n_texels * sizeof(float4));
    return PTC_OK;
  }
  { int rc = lm_debug_prepare(c); if (rc) return rc; }
  Lightmap& L = c->lightmap;
  int rc = ensure_buf(c, L.atlas[0], n_texels);
  if (!rc) rc = ensure_buf(c, L.atlas[1], n_texels);
  if (rc) return rc;
  hipStream_t st = c->lanes[0].stream;
  HIP_TRY(c, hipMemcpy(L.atlas[0].p, rgba_inout, n_texels * sizeof(float4), hipMemcpyHostToDevice));
  int cur = 0;
  for (int i = 0; i < iters; ++i) { pt_launch_lm_dilate(st, L.atlas[cur].p, L.atlas[cur ^ 1].p, width, height); cur ^= 1; }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipMemcpy(rgba_inout, L.atlas[cur].p, n_texels * sizeof(float4), hipMemcpyDeviceToHost));
  return PTC_OK;
}
}  // extern "C"
