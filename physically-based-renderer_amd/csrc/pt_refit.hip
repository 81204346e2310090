// pt_refit.hip — the refit of a committed scene on the device (see pt_refit.h).  The definition of every value is pt_scene_rules.h, which the host refit
// (ptc_refit_scene in ptc_scene.cpp) calls too; what is written here is who computes which value: threads, octets, reductions.
//
//   k_refit_flatten   one thread per world vertex: instance transform of position / normal / tangent / bitangent           (R1, vertex.glsl:28-40)
//   k_refit_prims     grid-stride over the primitives: the shading record of each, and the scene box by block reduction + 6 atomics per block
//   k_refit_nodes     one launch per level of the 8-wide tree, deepest first, one thread per node: child boxes (triangles of the leaf slots,
//                     the stored boxes of the interior children), node origin on the scene grid, 8-bit child planes, the triangle records of
//                     the leaf slots; the node keeps its slot masks and children block, a triangle record its primitive id and class
// All of it is HBM-bound byte shuffling with a few divisions per node: 48 B read + 60 B written per vertex, 3 gathers + 80 / 192 B written per
// primitive, 64 B + its triangles read and written per node.  No LDS tiling applies (every record is touched once), so the only layout rule is
// the one the arrays already obey: whole records per thread, threads in record order.
#include "pt_refit.h"
#include "pt_scene_rules.h"
using namespace scene_rules;

namespace {
constexpr int kBlock = 256;
constexpr int kNodeBlock = 64;

__global__ void k_refit_init(uint32_t* bounds) {
  const uint32_t i = threadIdx.x;
  if (i < 8) bounds[i] = i < 3 ? 0xffffffffu : 0u;
}

__global__ __launch_bounds__(kBlock) void k_refit_flatten(const DevRefit r) {
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= r.n_verts) return;
  const uint32_t inst = r.vert_inst[v];
  const float* m = r.inst_xf + (size_t)inst * 21;      // rows 0..2 of the model matrix column by column, then the normal matrix
  float bt[3];
  const HostVertex d = world_vertex(m, 3, m + 12, r.mesh_verts[r.inst_src[inst] + (v - r.inst_first[inst])], bt);
  r.wverts[v] = d;
  r.wbt[(size_t)v * 3 + 0] = bt[0]; r.wbt[(size_t)v * 3 + 1] = bt[1]; r.wbt[(size_t)v * 3 + 2] = bt[2];
  if (!(isfinite(d.position[0]) && isfinite(d.position[1]) && isfinite(d.position[2]))) atomicOr(&r.bounds[6], 1u);
}

__global__ __launch_bounds__(kBlock) void k_refit_prims(const DevRefit r) {
  if (r.bounds[6]) return;                 // a non-finite position: the host reports it, the scene in HBM stays as it was
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const bool tex = r.shade_stride == 12u;
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < r.n_tris; p += gridDim.x * kBlock) {
    const uint32_t vi[3] = {r.widx[(size_t)p * 3], r.widx[(size_t)p * 3 + 1], r.widx[(size_t)p * 3 + 2]};
    const HostVertex a = r.wverts[vi[0]], b = r.wverts[vi[1]], c = r.wverts[vi[2]];
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], fminf(a.position[k], fminf(b.position[k], c.position[k])));
      hi[k] = fmaxf(hi[k], fmaxf(a.position[k], fmaxf(b.position[k], c.position[k])));
    }
    float4* o = r.shade + (size_t)p * r.shade_stride;
    // material and emitter index of the primitive: not a refit's business
    shading_record(o, tex, a, b, c, r.wbt + (size_t)vi[0] * 3, r.wbt + (size_t)vi[1] * 3, r.wbt + (size_t)vi[2] * 3, __float_as_int(o[0].w), __float_as_int(o[1].w));
  }
  // scene box: min / max over finite values is the same number in any order (only the sign of a zero can differ, which nothing downstream reads)
  __shared__ float red[6][kBlock / 64];
  for (int k = 0; k < 3; ++k) {
    for (int d = 32; d >= 1; d >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d)); }
    if ((threadIdx.x & 63) == 0) { red[k][threadIdx.x >> 6] = lo[k]; red[3 + k][threadIdx.x >> 6] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < kBlock / 64; ++w) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    if (threadIdx.x < 3) { if (v != INFINITY) atomicMin(&r.bounds[threadIdx.x], ordered_u(v)); }
    else if (v != -INFINITY) atomicMax(&r.bounds[threadIdx.x], ordered_u(v));
  }
}

// the triangle whose record starts at unit `at` (the record's word 3 is its primitive id, word 7 its class: kept): its record rewritten, its box returned
__device__ inline Box refit_triangle(const DevRefit& r, uint32_t at) {
  const uint32_t prim = __float_as_uint(r.recs[at].w);
  const float* a = r.wverts[r.widx[(size_t)prim * 3 + 0]].position;
  const float* b = r.wverts[r.widx[(size_t)prim * 3 + 1]].position;
  const float* c = r.wverts[r.widx[(size_t)prim * 3 + 2]].position;
  const Box t = triangle_box(a, b, c);
  tri_record(r.recs + at, a, b, c, prim, __float_as_uint(r.recs[at + 1].w));
  return t;
}

// EIGHT lanes per node, one per child slot (round 4, second session).  One thread per node walked its eight slots one after the other: up to 16 triangles behind three dependent
// loads each (record -> vertex index -> vertex) and ~60 correctly rounded divisions, 20-50 us per LEVEL whatever its size — 0.35 of the refit's 0.5 ms.  Now lane s of an octet
// loads the box of slot s (an interior child's stored box, or its one or two triangles, whose records it rewrites), the octet exchanges the eight boxes (48 shuffles), every lane
// derives the node's box, origin and first exponent from them — the arithmetic and the order of the one-thread version, so the bytes are the same —, and in the exponent search lane
// s quantises slot s; the octet's verdict is a byte of a ballot.  Lane 0 packs and writes the node.
__global__ __launch_bounds__(kNodeBlock) void k_refit_nodes(const DevRefit r, uint32_t first, uint32_t count, float glx, float gly, float glz, float gsx, float gsy, float gsz, float scene_area) {
  const uint32_t t = blockIdx.x * kNodeBlock + threadIdx.x;
  const uint32_t i = t >> 3, sl = t & 7u;
  const int oct0 = (int)(threadIdx.x & 63u & ~7u);          // first lane of this octet inside the wave
  const bool live = i < count;                             // uniform over an octet
  unsigned long long my_cost = 0ull;
  uint32_t addr = 0, imask = 0, lmask = 0, two = 0, block = 0, masks = 0;
  if (live) {
    addr = r.level_nodes[first + i];
    const uint4 head = reinterpret_cast<const uint4*>(r.recs)[addr];
    imask = (head.z >> 8) & 255u; lmask = (head.z >> 16) & 255u; two = (head.z >> 24) & 255u; block = head.w; masks = node_masks_of(head.z);
  }
  const uint32_t used = imask | lmask;
  const bool mine = ((used >> sl) & 1u) != 0u;
  Box b = empty_box();
  if ((imask >> sl) & 1u) {
    const uint32_t child = block + 4u * (uint32_t)__popc(imask & ((1u << sl) - 1u));
    const float* nb = r.nbox + (size_t)(child >> 2) * 6;
    for (int k = 0; k < 3; ++k) { b.lo[k] = nb[k]; b.hi[k] = nb[3 + k]; }
  } else if ((lmask >> sl) & 1u) {
    const uint32_t below = (1u << sl) - 1u;
    const uint32_t tris_below = (uint32_t)__popc(lmask & below) + (uint32_t)__popc(two & lmask & below);
    const uint32_t at = block + 4u * (uint32_t)__popc(imask) + 3u * tris_below;
    b = refit_triangle(r, at);
    if ((two >> sl) & 1u) grow(b, refit_triangle(r, at + 3u));
  }
  // the eight boxes of the node, in every lane of its octet
  float clo[3][8], chi[3][8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) { clo[k][j] = __shfl(b.lo[k], oct0 + j); chi[k][j] = __shfl(b.hi[k], oct0 + j); }
  const float glo[3] = {glx, gly, glz}, gstep[3] = {gsx, gsy, gsz};
  uint32_t oq[3], e3[3], wlo[3][2], whi[3][2];
  float nbx[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float nlo = 0.0f, nhi = 0.0f;
    bool have = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!((used >> j) & 1u)) continue;
      if (!have) { nlo = clo[k][j]; nhi = chi[k][j]; have = true; }
      else { nlo = clo[k][j] < nlo ? clo[k][j] : nlo; nhi = chi[k][j] > nhi ? chi[k][j] : nhi; }
    }
    nbx[k] = nlo; nbx[3 + k] = nhi;
    oq[k] = grid_origin(nlo, glo[k], gstep[k]);
    const float org = grid_point(oq[k], glo[k], gstep[k]);
    uint32_t e = first_plane_exponent(nhi, org);
    bool done = !live;
    uint32_t ql = 255u, qh = 0u;           // an empty slot
    for (;;) {
      bool ok = true;
      if (!done && mine) {
        const Planes q = quantize_planes(b.lo[k], b.hi[k], org, e);
        ql = q.ql; qh = q.qh; ok = q.fits;
      }
      const unsigned long long verdict = __ballot(done || ok);
      if (!done) { if (((verdict >> oct0) & 0xffull) == 0xffull) done = true; else ++e; }
      if (!__ballot(!done)) break;
    }
    e3[k] = e;
    uint32_t pl[8], ph[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { pl[j] = (uint32_t)__shfl((int)ql, oct0 + j); ph[j] = (uint32_t)__shfl((int)qh, oct0 + j); }
    wlo[k][0] = pack4(pl[0], pl[1], pl[2], pl[3]); wlo[k][1] = pack4(pl[4], pl[5], pl[6], pl[7]);
    whi[k][0] = pack4(ph[0], ph[1], ph[2], ph[3]); whi[k][1] = pack4(ph[4], ph[5], ph[6], ph[7]);
  }
  if (live && sl == 0u) {
    uint4* out = reinterpret_cast<uint4*>(r.recs) + addr;
    uint32_t w[3];
    node_header(oq, e3, masks, w);
    out[0] = make_uint4(w[0], w[1], w[2], block);
    out[1] = make_uint4(wlo[0][0], wlo[0][1], wlo[1][0], wlo[1][1]);
    out[2] = make_uint4(wlo[2][0], wlo[2][1], whi[0][0], whi[0][1]);
    out[3] = make_uint4(whi[1][0], whi[1][1], whi[2][0], whi[2][1]);
    float* nb = r.nbox + (size_t)(addr >> 2) * 6;
    for (int k = 0; k < 6; ++k) nb[k] = nbx[k];
  }
  // surface-area cost of this node's children (ptc_stats.bvh_sa_cost): one term per used slot
  if (live && mine && scene_area > 0.0f) my_cost = sa_cost_term(b, scene_area, ((two >> sl) & 1u) != 0u);
  // one atomic per wave (a block is one wave): integer sum, the same bits in any order
  for (int d = 32; d >= 1; d >>= 1) my_cost += __shfl_xor(my_cost, d);
  if ((threadIdx.x & 63) == 0 && my_cost) atomicAdd(r.cost, my_cost);
}
}  // namespace

// A commit on the device starts from shading records that hold nothing but their two indices (k_refit_prims writes the rest around them).
namespace {
__global__ __launch_bounds__(kBlock) void k_refit_seed(float4* shade, uint32_t stride, const int32_t* tri_mat, const int32_t* prim_light, uint32_t n) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  float4* o = shade + (size_t)p * stride;
  o[0].w = __int_as_float(tri_mat[p]);
  o[1].w = __int_as_float(prim_light[p]);
}
}  // namespace
void pt_launch_refit_seed(hipStream_t st, const DevRefit& r, const int32_t* tri_mat, const int32_t* prim_light) {
  if (r.n_tris) hipLaunchKernelGGL(k_refit_seed, dim3((r.n_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, st, r.shade, r.shade_stride, tri_mat, prim_light, r.n_tris);
}

void pt_launch_refit_geometry(hipStream_t st, const DevRefit& r) {
  hipLaunchKernelGGL(k_refit_init, dim3(1), dim3(64), 0, st, r.bounds);
  if (r.n_verts) hipLaunchKernelGGL(k_refit_flatten, dim3((r.n_verts + kBlock - 1) / kBlock), dim3(kBlock), 0, st, r);
  uint32_t blocks = (r.n_tris + kBlock - 1) / kBlock;
  if (blocks > 1024u) blocks = 1024u;
  if (blocks) hipLaunchKernelGGL(k_refit_prims, dim3(blocks), dim3(kBlock), 0, st, r);
}

void pt_refit_decode_bounds(const uint32_t raw[8], float lo[3], float hi[3], bool* non_finite) {
  for (int k = 0; k < 6; ++k) (k < 3 ? lo[k] : hi[k - 3]) = unordered_f(raw[k]);
  *non_finite = raw[6] != 0u;
}

void pt_launch_refit_nodes(hipStream_t st, const DevRefit& r, const std::vector<uint32_t>& level_first, const float gl[3], const float gs[3], float scene_area) {
  (void)hipMemsetAsync(r.cost, 0, sizeof(unsigned long long), st);
  for (size_t l = 0; l + 1 < level_first.size(); ++l) {
    const uint32_t first = level_first[l], count = level_first[l + 1] - first;
    if (!count) continue;
    hipLaunchKernelGGL(k_refit_nodes, dim3((count * 8u + kNodeBlock - 1) / kNodeBlock), dim3(kNodeBlock), 0, st, r, first, count, gl[0], gl[1], gl[2], gs[0], gs[1], gs[2], scene_area);      // eight lanes per node
  }
}
