// pt_lightmap.hip — the kernels of a lightmap frame (see pt_lightmap.h; the definition of every value is there, and the host evaluation calls it too).
//
//   k_lm_cover        one 64-lane wave per triangle of the instance: the lanes stride the texels of the triangle's clamped bounding box and take the minimum of the
//                     primitive index into the owner image (cleared to 0xffffffff) with an integer atomicMin — a minimum does not depend on the order, which is why
//                     it may be an atomic.  The consumer is a later launch: no fence protocol.
//   k_lm_flag_count   one thread per texel: owned, and the owner's world triangle has a finite face normal -> a flag byte; kept texels per block, dropped texels
//   k_lm_scan         one block: the per-block counts -> their exclusive prefix, the total (pt_adaptive.hip's scan)
//   k_lm_list         the kept texels to their places — block prefix + the waves before + the kept lanes before: a stable compaction, ascending atlas index
//   k_lm_texels       one thread per entry: the owner's edge values at the centre again, barycentrics, P, n, the origin; two 16-byte stores
//   k_raygen_texel    one thread per path, k_raygen_probe's grid and queue bytes: two 16-byte loads of the entry's record, four coalesced 16-byte stores
//   k_lm_first_hit    bounce 0 only, between closest(0) and shade(0): one wave per segment of the ray queue (pt_pass_common.h); the hit record and the ray
//                     are read only; back[path % n] += 1 where the face normal of the hit primitive looks along the ray.  Integer atomicAdd: the count does not
//                     depend on the order.  Nothing another kernel of the batch reads is written
//   k_lm_scatter      one thread per entry: E = sum * (pi / N) to the entry's texel with alpha 1, nothing for an invalid entry
//   k_lm_dilate       one thread per texel, one iteration, ping-pong
// No float atomic anywhere.  profiles/lightmap_atrium.txt has the kernels' times against their byte floors.
#include "pt_lightmap.h"
#include "pt_pass_common.h"

namespace {
#define LM_WAVES (PT_LM_BLOCK / 64u)      // k_lm_cover's wave per triangle, and the per-wave sums of a block
#define LM_SCAN_BLOCK 1024

struct LmCorners { uint32_t i0, i1, i2; };
PT_DEV LmCorners lm_corners(const DevLmGeom& g, uint32_t tri) {
  LmCorners c;
  c.i0 = g.widx[(size_t)tri * 3u] - g.vert_first; c.i1 = g.widx[(size_t)tri * 3u + 1u] - g.vert_first; c.i2 = g.widx[(size_t)tri * 3u + 2u] - g.vert_first;
  return c;
}
PT_DEV pt_lm_tri lm_tri(const DevLmGeom& g, const LmCorners& c) {
  const float a[2] = {g.uv[(size_t)c.i0 * 2u], g.uv[(size_t)c.i0 * 2u + 1u]}, b[2] = {g.uv[(size_t)c.i1 * 2u], g.uv[(size_t)c.i1 * 2u + 1u]};
  const float d[2] = {g.uv[(size_t)c.i2 * 2u], g.uv[(size_t)c.i2 * 2u + 1u]};
  return pt_lm_make_tri(a, b, d, g.w, g.h);
}
PT_DEV v3 lm_pos(const DevLmGeom& g, uint32_t i) { return V3(g.verts[i].position); }
PT_DEV v3 lm_nrm(const DevLmGeom& g, uint32_t i) { return V3(g.verts[i].normal); }

__global__ __launch_bounds__(PT_LM_BLOCK) void k_lm_cover(DevLmGeom g, uint32_t* __restrict__ owner) {
  const uint32_t lane = threadIdx.x & 63u, tri = blockIdx.x * LM_WAVES + (threadIdx.x >> 6);
  if (tri >= g.n_tris) return;
  const pt_lm_tri t = lm_tri(g, lm_corners(g, tri));
  if (t.area == 0) return;
  int x0, x1, y0, y1;
  pt_lm_box(t, g.w, g.h, x0, x1, y0, y1);      // inside [0, w - 1] x [0, h - 1]
  if (x0 > x1 || y0 > y1) return;
  const uint32_t bw = (uint32_t)(x1 - x0 + 1), total = bw * (uint32_t)(y1 - y0 + 1);      // <= w h <= 2^26
  for (uint32_t i = lane; i < total; i += 64u) {
    const int x = x0 + (int)(i % bw), y = y0 + (int)(i / bw);
    int64_t e[3];
    if (pt_lm_edges(t, x, y, e)) atomicMin(&owner[(size_t)y * (size_t)g.w + (size_t)x], tri);
  }
}

__global__ __launch_bounds__(PT_LM_BLOCK) void k_lm_flag_count(DevLmGeom g, const uint32_t* __restrict__ owner, uint8_t* __restrict__ flags, uint32_t* __restrict__ block_tot,
                                                               uint32_t* __restrict__ counts, uint32_t n_texels) {
  __shared__ uint32_t s_k[LM_WAVES], s_d[LM_WAVES];
  const uint32_t a = blockIdx.x * PT_LM_BLOCK + threadIdx.x;
  bool keep = false, drop = false;
  if (a < n_texels) {
    const uint32_t tri = owner[a];
    if (tri != PT_LM_NONE) {
      const LmCorners c = lm_corners(g, tri);
      keep = pt_lm_finite3(pt_lm_face_normal(lm_pos(g, c.i0), lm_pos(g, c.i1), lm_pos(g, c.i2)));
      drop = !keep;
    }
    flags[a] = keep ? 1 : 0;
  }
  const unsigned long long bk = __ballot(keep), bd = __ballot(drop);
  if ((threadIdx.x & 63u) == 0) { s_k[threadIdx.x >> 6] = (uint32_t)__popcll(bk); s_d[threadIdx.x >> 6] = (uint32_t)__popcll(bd); }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t k = 0, d = 0;
    for (uint32_t i = 0; i < LM_WAVES; ++i) { k += s_k[i]; d += s_d[i]; }
    block_tot[blockIdx.x] = k;
    if (d) atomicAdd(&counts[1], d);      // an integer sum: the order does not matter
  }
}

// one block: block_tot[0, n_blocks) -> its exclusive prefix in place, the total to counts[0]
__global__ __launch_bounds__(LM_SCAN_BLOCK) void k_lm_scan(uint32_t n_blocks, uint32_t* __restrict__ block_tot, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_w[LM_SCAN_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_blocks; base += LM_SCAN_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_blocks ? block_tot[i] : 0u;
    uint32_t incl = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63u) s_w[wid] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t k = 0; k < LM_SCAN_BLOCK / 64; ++k) { const uint32_t t = s_w[k]; if (k < wid) before += t; all += t; }
    if (i < n_blocks) block_tot[i] = carry + before + (incl - v);
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[0] = carry;
}

__global__ __launch_bounds__(PT_LM_BLOCK) void k_lm_list(uint32_t n_texels, const uint8_t* __restrict__ flags, const uint32_t* __restrict__ block_pre, uint32_t* __restrict__ list) {
  __shared__ uint32_t s_w[LM_WAVES];
  const uint32_t a = blockIdx.x * PT_LM_BLOCK + threadIdx.x;
  const bool k = a < n_texels && flags[a] != 0;
  const unsigned long long b = __ballot(k);
  const uint32_t in_wave = mbcnt64(b), wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) s_w[wid] = (uint32_t)__popcll(b);
  __syncthreads();
  if (!k) return;
  uint32_t dst = block_pre[blockIdx.x] + in_wave;
  for (uint32_t i = 0; i < wid; ++i) dst += s_w[i];
  if (dst >= n_texels) return;      // cannot happen (a prefix of kept texels of n_texels): the list holds n_texels words
  list[dst] = a;
}

__global__ __launch_bounds__(PT_LM_BLOCK) void k_lm_texels(DevLmGeom g, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ list, uint32_t n_entries, float ray_eps,
                                                           float4* __restrict__ texels) {
  const uint32_t e = blockIdx.x * PT_LM_BLOCK + threadIdx.x;
  if (e >= n_entries) return;
  const uint32_t a = list[e], tri = owner[a];
  const LmCorners c = lm_corners(g, tri);
  const pt_lm_tri t = lm_tri(g, c);
  int64_t ev[3];
  pt_lm_edges(t, (int)(a % (uint32_t)g.w), (int)(a / (uint32_t)g.w), ev);
  v3 o, n;
  pt_lm_texel(ev, lm_pos(g, c.i0), lm_pos(g, c.i1), lm_pos(g, c.i2), lm_nrm(g, c.i0), lm_nrm(g, c.i1), lm_nrm(g, c.i2), ray_eps, o, n);
  texels[(size_t)e * 2u] = make_float4(o.x, o.y, o.z, __uint_as_float(a));
  texels[(size_t)e * 2u + 1u] = make_float4(n.x, n.y, n.z, __uint_as_float(tri));
}

__global__ __launch_bounds__(256) void k_raygen_texel(const float4* __restrict__ texels, uint32_t n_entries, uint32_t base, uint32_t seed_hash, DevQueues q, uint32_t first_sample,
                                                      uint32_t n_paths) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_paths) return;
  const uint32_t e = p % n_entries, sl = p / n_entries;
  const float4 T0 = texels[(size_t)e * 2u], T1 = texels[(size_t)e * 2u + 1u];
  float d[3];
  uint32_t key;
  pt_lm_dir(seed_hash, base + __float_as_uint(T0.w), first_sample + sl, V3(T1.x, T1.y, T1.z), d, key);
  store_primary_ray(q, p, V3(T0.x, T0.y, T0.z), V3(d), key, true);
}

__global__ __launch_bounds__(WALK_BLOCK) void k_lm_first_hit(DevScene sc, DevQueues q, int qi, uint32_t n_entries, uint32_t* __restrict__ back) {
  const uint32_t lane = lane_id();
  const WaveSegment w = wave_segment(q);
  if (!w.owned) return;
  const RayQ rin = q.ray[qi];
  const uint32_t first = w.base(q), n = w.count(q.seg_ray[qi]);
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    if (i0 + lane >= n) continue;
    const uint32_t slot = first + i0 + lane;
    const float4 H = q.hit[slot];
    const int32_t pc = __float_as_int(H.y);
    if (pc < 0) continue;                                       // a miss
    const float4 A = rin.A[slot], B = rin.B[slot], C = rin.C[slot];
    const float4* rec = sc.shade + (size_t)((uint32_t)pc & 0x0fffffffu) * sc.shade_stride;
    const v3 ng = record_face_normal(rec[0], rec[1], rec[2]);
    if (dot3(ng, V3(A.w, B.x, B.y)) > 0.0f) atomicAdd(&back[__float_as_uint(C.z) % n_entries], 1u);
  }
}

__global__ __launch_bounds__(PT_LM_BLOCK) void k_lm_scatter(const float4* __restrict__ texels, uint32_t n_entries, const float4* __restrict__ accum, const uint32_t* __restrict__ back,
                                                            uint32_t n_samples, float threshold, float4* __restrict__ atlas, float* __restrict__ out_back) {
  const uint32_t e = blockIdx.x * PT_LM_BLOCK + threadIdx.x;
  if (e >= n_entries) return;
  const uint32_t a = __float_as_uint(texels[(size_t)e * 2u].w), bk = back[e];
  if (out_back) out_back[e] = (float)bk / (float)n_samples;
  if (pt_lm_invalid(bk, n_samples, threshold)) return;          // enters the dilation as empty: the atlas was cleared
  const float4 s = accum[e];
  const float k = pt_lm_resolve_scale(n_samples);
  atlas[a] = make_float4(s.x * k, s.y * k, s.z * k, 1.0f);
}

__global__ __launch_bounds__(PT_LM_BLOCK) void k_lm_dilate(const float4* __restrict__ in, float4* __restrict__ out, int w, int h) {
  const uint32_t a = blockIdx.x * PT_LM_BLOCK + threadIdx.x;
  if (a >= (uint32_t)w * (uint32_t)h) return;
  out[a] = pt_lm_dilate(in, w, h, (int)(a % (uint32_t)w), (int)(a / (uint32_t)w));
}
}  // namespace

void pt_launch_lm_cover(hipStream_t s, const DevLmGeom& g, uint32_t* owner) {
  (void)hipMemsetAsync(owner, 0xff, (size_t)g.w * (size_t)g.h * sizeof(uint32_t), s);
  if (!g.n_tris) return;
  hipLaunchKernelGGL(k_lm_cover, dim3((g.n_tris + LM_WAVES - 1u) / LM_WAVES), dim3(PT_LM_BLOCK), 0, s, g, owner);
}

void pt_launch_lm_list(hipStream_t s, const DevLmGeom& g, const uint32_t* owner, const DevLmScratch& sc, uint32_t* list) {
  const uint32_t n = (uint32_t)g.w * (uint32_t)g.h, nb = pt_lm_blocks(n);
  (void)hipMemsetAsync(sc.counts, 0, 2 * sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_lm_flag_count, dim3(nb), dim3(PT_LM_BLOCK), 0, s, g, owner, sc.flags, sc.block_tot, sc.counts, n);
  hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LM_SCAN_BLOCK), 0, s, nb, sc.block_tot, sc.counts);
  hipLaunchKernelGGL(k_lm_list, dim3(nb), dim3(PT_LM_BLOCK), 0, s, n, (const uint8_t*)sc.flags, (const uint32_t*)sc.block_tot, list);
}

void pt_launch_lm_texels(hipStream_t s, const DevLmGeom& g, const uint32_t* owner, const uint32_t* list, uint32_t n_entries, float ray_eps, float4* texels) {
  if (!n_entries) return;
  hipLaunchKernelGGL(k_lm_texels, dim3(pt_lm_blocks(n_entries)), dim3(PT_LM_BLOCK), 0, s, g, owner, list, n_entries, ray_eps, texels);
}

void pt_launch_raygen_texel(hipStream_t s, const float4* texels, uint32_t n_entries, uint32_t index_base, uint32_t seed_hash, const DevQueues& q, uint32_t first_sample,
                            uint32_t n_samples) {
  const uint32_t n_paths = n_entries * n_samples;
  if (!n_paths) return;
  hipLaunchKernelGGL(k_raygen_texel, dim3((n_paths + 255u) / 256u), dim3(256), 0, s, texels, n_entries, index_base, seed_hash, q, first_sample, n_paths);
}

void pt_launch_lm_first_hit(hipStream_t s, const DevScene& sc, const DevQueues& q, int qi, uint32_t n_entries, uint32_t* back) {
  if (!n_entries) return;
  hipLaunchKernelGGL(k_lm_first_hit, walk_grid(q), dim3(WALK_BLOCK), 0, s, sc, q, qi, n_entries, back);
}

void pt_launch_lm_scatter(hipStream_t s, const float4* texels, uint32_t n_entries, const float4* accum, const uint32_t* back, uint32_t n_samples, float threshold, float4* atlas,
                          float* out_back) {
  if (!n_entries || !n_samples) return;
  hipLaunchKernelGGL(k_lm_scatter, dim3(pt_lm_blocks(n_entries)), dim3(PT_LM_BLOCK), 0, s, texels, n_entries, accum, back, n_samples, threshold, atlas, out_back);
}

void pt_launch_lm_dilate(hipStream_t s, const float4* in, float4* out, int w, int h) {
  hipLaunchKernelGGL(k_lm_dilate, dim3(pt_lm_blocks((uint32_t)w * (uint32_t)h)), dim3(PT_LM_BLOCK), 0, s, in, out, w, h);
}
