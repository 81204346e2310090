// pt_build.hip — the LBVH and binned-SAH builds on the device (see pt_build.h).
//
// Everything here is integer / byte work with a few float comparisons per node: HBM- and latency-bound, nothing for MFMA.  The arithmetic that decides
// the tree — centres, Morton quantisation, box unions, half areas, bin indices, cut costs, the collapse tables, the slot scores — is pt_scene_rules.h's, the
// text the host build (ptc_scene.cpp) runs too, because the contract is byte equality of the result, not a tree "as good as" the host's.  What is written
// here is how the work is spread: sorts, scans, levels, and the layout (which the host numbers by another algorithm to the same addresses).
#include "pt_build.h"
#include "pt_scene_rules.h"
using namespace scene_rules;

#include <string>
#include <vector>

namespace {
constexpr int kBlock = 256;
constexpr uint32_t kEmptyLink = 0x80000000u;
constexpr uint32_t kUnset = 0xffffffffu;
constexpr uint32_t kSortTile = 512;       // keys per wave of a sort pass: 8 steps of 64, in order (the sort is stable)

struct Bld {
  const HostVertex* wverts; const uint32_t* widx; const uint32_t* prim_cls; uint32_t n, budget;
  Box* tbox; uint32_t* cb;
  unsigned long long *key_a, *key_b; uint32_t *val_a, *val_b; uint32_t* hist; uint32_t* digit_total;
  int32_t *r_left, *r_right; uint32_t *r_lo, *r_hi, *r_parent, *leaf_parent, *r_flag;
  Box* r_box; DpT* dp;
  int32_t* w_radix; uint32_t* w_parent; int32_t* w_link; uint32_t* w_child; uint32_t *w_own, *w_sub, *w_baddr, *w_naddr;
  uint32_t* counters;    // [0] 8-wide nodes so far, [1] units of the array, [2] entries of top_order
  uint32_t* top_order;
  // the binned-SAH front end (k_sah_*): centres, the open ranges of a level (small: one wave each; big: several workgroups each) double-buffered by level parity,
  // their counts per level, the big ranges' global bins, per-workgroup left counts, the root's cut
  float4* ctr; struct SahRange *s_list[2], *s_big[2]; uint32_t *s_cnt, *s_bigcnt; struct SahSlot* s_slot; uint32_t *s_blk, *s_root;   // s_root[1]: error bits
};

__global__ void k_bld_init(Bld b) {
  const uint32_t i = threadIdx.x;
  if (i < 6) b.cb[i] = i < 3 ? 0xffffffffu : 0u;
  if (i == 0) { b.counters[0] = 1u; b.counters[1] = 0u; b.counters[2] = 0u; b.w_radix[0] = 0; b.w_parent[0] = kUnset; }
}

// ---- triangle boxes and the bounds of their centres -------------------------
__global__ __launch_bounds__(kBlock) void k_bld_prims(Bld b) {
  float cl[3] = {INFINITY, INFINITY, INFINITY}, ch[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < b.n; p += gridDim.x * kBlock) {
    const Box t = triangle_box(b.wverts[b.widx[(size_t)p * 3]].position, b.wverts[b.widx[(size_t)p * 3 + 1]].position, b.wverts[b.widx[(size_t)p * 3 + 2]].position);
    b.tbox[p] = t;
    for (int k = 0; k < 3; ++k) { const float c = centre(t, k); cl[k] = fminf(cl[k], c); ch[k] = fmaxf(ch[k], c); }
  }
  __shared__ float red[6][kBlock / 64];
  for (int k = 0; k < 3; ++k) {
    for (int d = 32; d >= 1; d >>= 1) { cl[k] = fminf(cl[k], __shfl_xor(cl[k], d)); ch[k] = fmaxf(ch[k], __shfl_xor(ch[k], d)); }
    if ((threadIdx.x & 63) == 0) { red[k][threadIdx.x >> 6] = cl[k]; red[3 + k][threadIdx.x >> 6] = ch[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[threadIdx.x][0];
    for (int w = 1; w < kBlock / 64; ++w) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
    if (threadIdx.x < 3) { if (v != INFINITY) atomicMin(&b.cb[threadIdx.x], ordered_u(v)); }
    else if (v != -INFINITY) atomicMax(&b.cb[threadIdx.x], ordered_u(v));
  }
}

__global__ __launch_bounds__(kBlock) void k_bld_codes(Bld b) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= b.n) return;
  const Box t = b.tbox[p];
  unsigned long long code = 0;
  for (int k = 0; k < 3; ++k) {
    const float cl = unordered_f(b.cb[k]);
    code |= morton_axis(centre(t, k), cl, cell_scale(cl, unordered_f(b.cb[3 + k]), kMortonCells)) << k;
  }
  b.key_a[p] = code; b.val_a[p] = p;
}

// ---- LSD radix sort, 8 bits per pass.  A wave owns a tile of kSortTile consecutive keys and takes them 64 at a time, in order; the rank of a key among
// the earlier keys of its tile with the same digit is (the tile's running count of that digit) + (lanes below it with that digit: 8 ballots intersected,
// then mbcnt) — stable, no atomics on the output side, no sort inside the tile.
__device__ inline uint32_t lane_of() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ inline uint32_t mbcnt_u64(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
__device__ inline void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__global__ __launch_bounds__(kBlock) void k_sort_hist(const unsigned long long* keys, uint32_t n, int shift, uint32_t* hist) {
  __shared__ uint32_t h[kBlock / 64][256];
  const uint32_t wave = threadIdx.x >> 6, lane = lane_of();
  for (uint32_t i = lane; i < 256u; i += 64u) h[wave][i] = 0u;
  wave_sync_lds();
  const uint32_t tile = blockIdx.x * (kBlock / 64) + wave;
  const size_t base = (size_t)tile * kSortTile;
  for (uint32_t s = 0; s < kSortTile; s += 64u) {
    const size_t i = base + s + lane;
    if (i < n) atomicAdd(&h[wave][(uint32_t)(keys[i] >> shift) & 255u], 1u);
  }
  wave_sync_lds();
  if (base < n) for (uint32_t i = lane; i < 256u; i += 64u) hist[(size_t)tile * 256u + i] = h[wave][i];
}
// hist[tile][digit] -> the first output position of that digit of that tile: digits ascending, tiles ascending inside a digit.  k_sort_scan_tiles: block d
// turns digit d's column into its exclusive prefix over the tiles (256 tiles per round, wave shuffles + one LDS exchange) and leaves the column's total;
// k_sort_scan_digits: exclusive prefix of the 256 totals — the scatter adds the two.
__global__ __launch_bounds__(256) void k_sort_scan_tiles(uint32_t* hist, uint32_t tiles, uint32_t* total) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t carry_s;
  const uint32_t d = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0u;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < tiles; t0 += 256u) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < tiles ? hist[(size_t)t * 256u + d] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if ((int)lane >= o) inc += u; }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    if (t < tiles) hist[(size_t)t * 256u + d] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == 255u) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) total[d] = carry_s;
}
__global__ __launch_bounds__(256) void k_sort_scan_digits(uint32_t* total) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t v = total[threadIdx.x];
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if ((int)lane >= o) inc += u; }
  if (lane == 63u) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
  total[threadIdx.x] = before + inc - v;
}
__global__ __launch_bounds__(kBlock) void k_sort_scatter(const unsigned long long* keys, const uint32_t* vals, uint32_t n, int shift, const uint32_t* offs, const uint32_t* digit_base,
                                                         unsigned long long* keys_out, uint32_t* vals_out) {
  __shared__ uint32_t cnt[kBlock / 64][256];
  const uint32_t wave = threadIdx.x >> 6, lane = lane_of();
  const uint32_t tile = blockIdx.x * (kBlock / 64) + wave;
  const size_t base = (size_t)tile * kSortTile;
  if (base >= n) return;
  for (uint32_t i = lane; i < 256u; i += 64u) cnt[wave][i] = digit_base[i] + offs[(size_t)tile * 256u + i];
  wave_sync_lds();
  for (uint32_t s = 0; s < kSortTile; s += 64u) {
    const size_t i = base + s + lane;
    const bool valid = i < n;
    const unsigned long long key = valid ? keys[i] : 0ull;
    const uint32_t val = valid ? vals[i] : 0u;
    const uint32_t dg = (uint32_t)(key >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = ((dg >> bit) & 1u) != 0u;
      const unsigned long long m = __ballot(on);
      peers &= on ? m : ~m;
    }
    const uint32_t rank = mbcnt_u64(peers);
    uint32_t pos = 0;
    if (valid) pos = cnt[wave][dg] + rank;
    wave_sync_lds();
    if (valid && rank == 0u) cnt[wave][dg] += (uint32_t)__popcll(peers);
    wave_sync_lds();
    if (valid) { keys_out[pos] = key; vals_out[pos] = val; }
  }
}

// ---- the radix tree of the keys (code, position): every internal node from the sorted codes alone (Karras 2012).  Internal node i covers [min(i, j), max(i, j)];
// node 0 is the root.  A child link >= 0 is an internal node, < 0 is ~(position of a single triangle) — the host's SplitNode.
__device__ inline int delta_keys(const unsigned long long* codes, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const unsigned long long a = codes[i], c = codes[j];
  if (a != c) return (int)__clzll((long long)(a ^ c));
  return 64 + (int)__clz((int)((uint32_t)i ^ (uint32_t)j));
}
__global__ __launch_bounds__(kBlock) void k_bld_radix(Bld b) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x), n = (int)b.n;
  if (i >= n - 1) return;
  const unsigned long long* codes = b.key_a;
  const int d = delta_keys(codes, n, i, i + 1) - delta_keys(codes, n, i, i - 1) > 0 ? 1 : -1;
  const int dmin = delta_keys(codes, n, i, i - d);
  int lmax = 2;
  while (delta_keys(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (delta_keys(codes, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta_keys(codes, n, i, j);
  int s = 0, t = l;
  do {
    t = (t + 1) / 2;
    if (delta_keys(codes, n, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int gamma = i + s * d + (d < 0 ? -1 : 0);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const int32_t left = lo == gamma ? ~gamma : gamma, right = hi == gamma + 1 ? ~(gamma + 1) : gamma + 1;
  b.r_left[i] = left; b.r_right[i] = right; b.r_lo[i] = (uint32_t)lo; b.r_hi[i] = (uint32_t)hi;
  if (left < 0) b.leaf_parent[gamma] = (uint32_t)i; else b.r_parent[gamma] = (uint32_t)i;
  if (right < 0) b.leaf_parent[gamma + 1] = (uint32_t)i; else b.r_parent[gamma + 1] = (uint32_t)i;
  if (i == 0) b.r_parent[0] = kUnset;
}

// ---- the binned-SAH binary tree (ptc_scene.cpp: build_split_tree, split_range, split_range_parallel), top down, one LEVEL of open ranges per launch.  Per range:
// the bounds of its centres come with it (its parent's partition reduced them); on every axis with ch > cl, 32 bins of j = min((int)((c - cl) * (32 / (ch - cl))), 31)
// hold a count and a box union (integer atomics: counts add, boxes take min / max of the order-preserving encoding — exact in any order); the suffix and prefix
// sweeps are lane scans of the same min / max and integer sums; each boundary's cost is sah_cut_cost; the cut is the first strict minimum in (axis, bin)
// order, or the middle when no axis has a candidate; the partition of ord[lo..hi] is stable on both sides.  So the tree is the host's, node for node.
// Node ids: an internal node is named by its cut (the last position of its left part), the root's cut swapped with 0 so that the root is node 0 — every id in
// [0, n - 2], no allocation; a child writes its own id into its parent's link when it is cut.
struct SahRange { uint32_t lo, hi, parent, bnd[6]; };     // parent: node id | side << 31 (kUnset for the root); bnd: ordered_u of the centre bounds lo[3], hi[3]
constexpr int kBinWords = 7 * 3 * kSahBins;               // [field][axis * 32 + bin]: field 0 the count, 1..3 box lo, 4..6 box hi (ordered_u)
constexpr uint32_t kSahBig = 1024;                        // ranges of at least this many triangles are cut by several workgroups (k_sah_big_*)
constexpr uint32_t kSahChunk = 4096;                      // triangles per workgroup of the big-range kernels
constexpr uint32_t kOrdPosInf = 0xff800000u, kOrdNegInf = 0x007fffffu;     // ordered_u(+inf), ordered_u(-inf)
struct SahSlot { uint32_t bins[kBinWords]; uint32_t cbnd[12]; int32_t axis, bin; };   // a big range's bins, its children's centre bounds (left lo/hi, right lo/hi), its cut
struct SahCut { int axis, bin; };

__device__ inline uint32_t sah_bin_init(uint32_t w) { return w < 3u * kSahBins ? 0u : (w < 12u * kSahBins ? kOrdPosInf : kOrdNegInf); }
__device__ inline uint32_t sah_cbnd_init(uint32_t w) { return (w % 6u) < 3u ? kOrdPosInf : kOrdNegInf; }
// the bin index addresses LDS and global atomics: a centre below its range's bounds (it cannot be: the bounds are the minima of these centres) stays in bin 0
__device__ inline int sah_bin_guarded(float c, float cl, float scale) { const int j = sah_bin(c, cl, scale); return j < 0 ? 0 : j; }
struct SahAxes {
  float cl[3], ch[3], scale[3];
  __device__ explicit SahAxes(const uint32_t* bnd) {
    for (int k = 0; k < 3; ++k) {
      cl[k] = unordered_f(bnd[k]); ch[k] = unordered_f(bnd[3 + k]);
      scale[k] = cell_scale(cl[k], ch[k], (float)kSahBins);
    }
  }
  __device__ bool on(int k) const { return ch[k] > cl[k]; }
};
// adds triangle p to the bins (LDS or global)
__device__ inline void sah_bin_add(uint32_t* bins, const SahAxes& ax, const float4& c, const Box& t) {
  const float cc[3] = {c.x, c.y, c.z};
  for (int k = 0; k < 3; ++k) {
    if (!ax.on(k)) continue;
    const uint32_t w = (uint32_t)k * kSahBins + (uint32_t)sah_bin_guarded(cc[k], ax.cl[k], ax.scale[k]);
    atomicAdd(&bins[w], 1u);
    for (int d = 0; d < 3; ++d) { atomicMin(&bins[(1 + d) * 3 * kSahBins + w], ordered_u(t.lo[d])); atomicMax(&bins[(4 + d) * 3 * kSahBins + w], ordered_u(t.hi[d])); }
  }
}
// The cut from complete bins, by one whole wave (every lane returns it): lane j holds bin j (lanes 32..63 empty bins), the sweeps are inclusive lane scans.
__device__ SahCut sah_choose(const uint32_t* bins, const SahAxes& ax) {
  const uint32_t lane = lane_of();
  float best = INFINITY; SahCut cut{-1, 0};
  for (int k = 0; k < 3; ++k) {
    if (!ax.on(k)) continue;
    uint32_t cnt = 0; Box bx = empty_box();
    if (lane < (uint32_t)kSahBins) {
      const uint32_t w = (uint32_t)k * kSahBins + lane;
      cnt = bins[w];
      for (int d = 0; d < 3; ++d) { bx.lo[d] = unordered_f(bins[(1 + d) * 3 * kSahBins + w]); bx.hi[d] = unordered_f(bins[(4 + d) * 3 * kSahBins + w]); }
    }
    uint32_t sc = cnt, pc = cnt; Box sb = bx, pb = bx;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t osc = __shfl_down(sc, o), opc = __shfl_up(pc, o);
      Box os, op;
      for (int d = 0; d < 3; ++d) {
        os.lo[d] = __shfl_down(sb.lo[d], o); os.hi[d] = __shfl_down(sb.hi[d], o);
        op.lo[d] = __shfl_up(pb.lo[d], o); op.hi[d] = __shfl_up(pb.hi[d], o);
      }
      if (lane + (uint32_t)o < 64u) { sc += osc; grow(sb, os); }
      if (lane >= (uint32_t)o) { pc += opc; grow(pb, op); }
    }
    const float sa = sah_suffix_area(sb, sc);                   // suffix_area[lane]
    const uint32_t nsc = __shfl_down(sc, 1);
    const float nsa = __shfl_down(sa, 1);
    float cost = INFINITY;
    if (lane + 1u < (uint32_t)kSahBins && pc != 0u && nsc != 0u) cost = sah_cut_cost(pb, pc, nsa, nsc);
    if (!(cost < INFINITY)) cost = INFINITY;                        // +inf and NaN never win
    int bj = (int)lane;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float oc = __shfl_xor(cost, o); const int oj = __shfl_xor(bj, o);
      if (oc < cost || (oc == cost && oj < bj)) { cost = oc; bj = oj; }
    }
    if (cost < best) { best = cost; cut.axis = k; cut.bin = bj; }
  }
  return cut;
}
__device__ inline bool sah_left(const SahCut& cut, const SahAxes& ax, const float4& c, uint32_t i, uint32_t mid) {
  if (cut.axis < 0) return i <= mid;
  const float cc = cut.axis == 0 ? c.x : (cut.axis == 1 ? c.y : c.z);
  return sah_bin_guarded(cc, ax.cl[cut.axis], ax.scale[cut.axis]) <= cut.bin;
}
__device__ inline void bnd_add(float* bd, const float4& c) {
  bd[0] = fminf(bd[0], c.x); bd[1] = fminf(bd[1], c.y); bd[2] = fminf(bd[2], c.z);
  bd[3] = fmaxf(bd[3], c.x); bd[4] = fmaxf(bd[4], c.y); bd[5] = fmaxf(bd[5], c.z);
}
__device__ inline void bnd_wave(float* bd) {
  for (int o = 32; o >= 1; o >>= 1)
    for (int d = 0; d < 3; ++d) { bd[d] = fminf(bd[d], __shfl_xor(bd[d], o)); bd[3 + d] = fmaxf(bd[3 + d], __shfl_xor(bd[3 + d], o)); }
}
__device__ void sah_push(const Bld& b, uint32_t lo, uint32_t hi, uint32_t parent, const float* bd, uint32_t level) {
  SahRange e;
  e.lo = lo; e.hi = hi; e.parent = parent;
  for (int d = 0; d < 6; ++d) e.bnd[d] = ordered_u(bd[d]);
  if (hi - lo + 1u >= kSahBig) b.s_big[level & 1u][atomicAdd(&b.s_bigcnt[level], 1u)] = e;
  else b.s_list[level & 1u][atomicAdd(&b.s_cnt[level], 1u)] = e;
}
// range r of `level` is cut after position g: its node, its link in its parent, its leaves, its children for the next level
__device__ void sah_finish(const Bld& b, const SahRange& r, uint32_t g, const float* lb, const float* rb, uint32_t level) {
  if (g < r.lo || g >= r.hi) { atomicOr(&b.s_root[1], 1u); g = r.lo + (r.hi - r.lo) / 2u; }      // cannot happen (both sides of a cut hold a triangle): reported, kept in bounds
  uint32_t id = 0;
  if (r.parent == kUnset) *b.s_root = g;
  else {
    const uint32_t g0 = *b.s_root;
    id = g == g0 ? 0u : (g == 0u ? g0 : g);
    if (r.parent >> 31) b.r_right[r.parent & 0x7fffffffu] = (int32_t)id; else b.r_left[r.parent] = (int32_t)id;
  }
  b.r_lo[id] = r.lo; b.r_hi[id] = r.hi;
  if (g == r.lo) b.r_left[id] = ~(int32_t)g; else sah_push(b, r.lo, g, id, lb, level + 1u);
  if (g + 1u == r.hi) b.r_right[id] = ~(int32_t)r.hi; else sah_push(b, g + 1u, r.hi, id | 0x80000000u, rb, level + 1u);
}

// centres, the identity order, the root range (its centre bounds are k_bld_prims')
__global__ __launch_bounds__(kBlock) void k_sah_init(Bld b) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= b.n) return;
  const Box t = b.tbox[p];
  b.ctr[p] = make_float4(centre(t, 0), centre(t, 1), centre(t, 2), 0.0f);
  b.val_a[p] = p;
  if (p == 0) {
    SahRange e;
    e.lo = 0; e.hi = b.n - 1u; e.parent = kUnset;
    for (int d = 0; d < 6; ++d) e.bnd[d] = b.cb[d];
    if (b.n >= kSahBig) { b.s_big[0][0] = e; b.s_bigcnt[0] = 1u; } else { b.s_list[0][0] = e; b.s_cnt[0] = 1u; }
  }
}
__global__ __launch_bounds__(kBlock) void k_sah_clear(Bld b, uint32_t slots) {
  constexpr uint32_t per = sizeof(SahSlot) / 4u;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < slots * per; i += gridDim.x * kBlock) {
    const uint32_t w = i % per;
    uint32_t* s = reinterpret_cast<uint32_t*>(b.s_slot);
    s[i] = w < (uint32_t)kBinWords ? sah_bin_init(w) : (w < (uint32_t)kBinWords + 12u ? sah_cbnd_init(w - (uint32_t)kBinWords) : 0u);
  }
}

// Every internal node written, every link and range in bounds (the back end follows them): else error bit 2.  r_left / r_right / r_hi start as 0x7f7f7f7f.
__global__ __launch_bounds__(kBlock) void k_sah_check(Bld b) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i + 1u >= b.n) return;
  const int32_t l = b.r_left[i], r = b.r_right[i];
  const uint32_t lo = b.r_lo[i], hi = b.r_hi[i];
  const auto ok = [&](int32_t k) { return k >= 0 ? (uint32_t)k + 1u < b.n : (uint32_t)~k < b.n; };
  if (!ok(l) || !ok(r) || hi >= b.n || lo >= hi) atomicOr(&b.s_root[1], 2u);
}

// Small ranges: one wave per range does everything — bins in LDS, the cut, the stable partition (left part in place: a left triangle is written at or below the
// position it was read from; right part to val_b, then back), the children's centre bounds.  Persistent: the waves stride over the level's list.
__global__ __launch_bounds__(kBlock) void k_sah_small(Bld b, uint32_t level) {
  __shared__ uint32_t sbins[kBlock / 64][kBinWords];
  const uint32_t wave = threadIdx.x >> 6, lane = lane_of();
  uint32_t* bins = sbins[wave];
  const uint32_t count = b.s_cnt[level];
  const SahRange* list = b.s_list[level & 1u];
  for (uint32_t e = blockIdx.x * (kBlock / 64) + wave; e < count; e += gridDim.x * (kBlock / 64)) {
    const SahRange r = list[e];
    const SahAxes ax(r.bnd);
    for (uint32_t w = lane; w < (uint32_t)kBinWords; w += 64u) bins[w] = sah_bin_init(w);
    wave_sync_lds();
    for (uint32_t i = r.lo + lane; i <= r.hi; i += 64u) { const uint32_t p = b.val_a[i]; sah_bin_add(bins, ax, b.ctr[p], b.tbox[p]); }
    wave_sync_lds();
    const SahCut cut = sah_choose(bins, ax);
    wave_sync_lds();                                            // the bins are read: the next range may clear them
    const uint32_t mid = r.lo + (r.hi - r.lo) / 2u;
    uint32_t nl = 0, nr = 0;
    float lb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY}, rb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (uint32_t base = r.lo; base <= r.hi; base += 64u) {
      const uint32_t i = base + lane;
      const bool valid = i <= r.hi;
      uint32_t p = 0; float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (valid) { p = b.val_a[i]; c = b.ctr[p]; }
      const bool left = valid && sah_left(cut, ax, c, i, mid), right = valid && !left;
      const unsigned long long ml = __ballot(left), mr = __ballot(right);
      if (cut.axis >= 0) {
        if (left) b.val_a[r.lo + nl + mbcnt_u64(ml)] = p;
        if (right) b.val_b[r.lo + nr + mbcnt_u64(mr)] = p;
      }
      nl += (uint32_t)__popcll(ml); nr += (uint32_t)__popcll(mr);
      if (left) bnd_add(lb, c);
      if (right) bnd_add(rb, c);
    }
    if (cut.axis >= 0) {
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();
      for (uint32_t k = lane; k < nr; k += 64u) b.val_a[r.lo + nl + k] = b.val_b[r.lo + k];
    }
    bnd_wave(lb); bnd_wave(rb);
    if (lane == 0u) sah_finish(b, r, r.lo + nl - 1u, lb, rb, level);
  }
}

// Big ranges: chunks of kSahChunk triangles, one workgroup each, over all big ranges of the level (the grid is an upper bound; the spare workgroups return).
// k_sah_big_bins: per-workgroup bins in LDS, merged into the range's slot; k_sah_big_count: the cut (every workgroup of the range makes it from the slot, the
// first one records it), left triangles per workgroup; k_sah_big_scatter: stable scatter into val_b (exclusive prefix over the range's earlier workgroups + rank
// in the chunk by ballot / mbcnt), the children's centre bounds; k_sah_big_finish: back to val_a, the first workgroup finishes the range and clears its slot.
__device__ inline bool sah_locate(const Bld& b, uint32_t level, uint32_t& r, uint32_t& first, SahRange& e) {
  const uint32_t nb = b.s_bigcnt[level];
  const SahRange* list = b.s_big[level & 1u];
  for (uint32_t k = 0, acc = 0; k < nb; ++k) {
    const uint32_t nblk = (list[k].hi - list[k].lo + kSahChunk) / kSahChunk;
    if (blockIdx.x < acc + nblk) { r = k; first = acc; e = list[k]; return true; }
    acc += nblk;
  }
  return false;
}
__global__ __launch_bounds__(kBlock) void k_sah_big_bins(Bld b, uint32_t level) {
  __shared__ uint32_t bins[kBinWords];
  uint32_t r, first; SahRange e;
  if (!sah_locate(b, level, r, first, e)) return;
  const SahAxes ax(e.bnd);
  for (uint32_t w = threadIdx.x; w < (uint32_t)kBinWords; w += kBlock) bins[w] = sah_bin_init(w);
  __syncthreads();
  const uint32_t a = e.lo + (blockIdx.x - first) * kSahChunk, z = min(a + kSahChunk - 1u, e.hi);
  for (uint32_t i = a + threadIdx.x; i <= z; i += kBlock) { const uint32_t p = b.val_a[i]; sah_bin_add(bins, ax, b.ctr[p], b.tbox[p]); }
  __syncthreads();
  uint32_t* g = b.s_slot[r].bins;
  for (uint32_t w = threadIdx.x; w < 3u * kSahBins; w += kBlock) {
    const uint32_t cnt = bins[w];
    if (!cnt) continue;
    atomicAdd(&g[w], cnt);
    for (int d = 0; d < 3; ++d) { atomicMin(&g[(1 + d) * 3 * kSahBins + w], bins[(1 + d) * 3 * kSahBins + w]); atomicMax(&g[(4 + d) * 3 * kSahBins + w], bins[(4 + d) * 3 * kSahBins + w]); }
  }
}
__global__ __launch_bounds__(kBlock) void k_sah_big_count(Bld b, uint32_t level) {
  __shared__ int cut_s[2];
  __shared__ uint32_t wl[kBlock / 64];
  uint32_t r, first; SahRange e;
  if (!sah_locate(b, level, r, first, e)) return;
  const SahAxes ax(e.bnd);
  if (threadIdx.x < 64u) {
    const SahCut cut = sah_choose(b.s_slot[r].bins, ax);
    if (threadIdx.x == 0) { cut_s[0] = cut.axis; cut_s[1] = cut.bin; if (blockIdx.x == first) { b.s_slot[r].axis = cut.axis; b.s_slot[r].bin = cut.bin; } }
  }
  __syncthreads();
  const SahCut cut{cut_s[0], cut_s[1]};
  const uint32_t mid = e.lo + (e.hi - e.lo) / 2u;
  const uint32_t a = e.lo + (blockIdx.x - first) * kSahChunk, z = min(a + kSahChunk - 1u, e.hi);
  uint32_t k = 0;
  for (uint32_t i = a + threadIdx.x; i <= z; i += kBlock) k += sah_left(cut, ax, b.ctr[b.val_a[i]], i, mid) ? 1u : 0u;
  for (int o = 32; o >= 1; o >>= 1) k += __shfl_xor(k, o);
  if (lane_of() == 0u) wl[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) { uint32_t s = 0; for (int w = 0; w < kBlock / 64; ++w) s += wl[w]; b.s_blk[blockIdx.x] = s; }
}
__global__ __launch_bounds__(kBlock) void k_sah_big_scatter(Bld b, uint32_t level) {
  __shared__ uint32_t base_s[2];
  __shared__ uint32_t wl[kBlock / 64], wr[kBlock / 64];
  uint32_t r, first; SahRange e;
  if (!sah_locate(b, level, r, first, e)) return;
  const SahAxes ax(e.bnd);
  const SahCut cut{b.s_slot[r].axis, b.s_slot[r].bin};
  const uint32_t nblk = (e.hi - e.lo + kSahChunk) / kSahChunk;
  if (threadIdx.x == 0) {
    uint32_t before = 0, total = 0;
    for (uint32_t k = 0; k < nblk; ++k) { const uint32_t v = b.s_blk[first + k]; if (first + k < blockIdx.x) before += v; total += v; }
    const uint32_t a = e.lo + (blockIdx.x - first) * kSahChunk;
    base_s[0] = e.lo + before; base_s[1] = e.lo + total + (a - e.lo - before);
  }
  __syncthreads();
  uint32_t lpos = base_s[0], rpos = base_s[1];
  const uint32_t wave = threadIdx.x >> 6, mid = e.lo + (e.hi - e.lo) / 2u;
  const uint32_t a = e.lo + (blockIdx.x - first) * kSahChunk, z = min(a + kSahChunk - 1u, e.hi);
  float lb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY}, rb[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (uint32_t base = a; base <= z; base += kBlock) {
    const uint32_t i = base + threadIdx.x;
    const bool valid = i <= z;
    uint32_t p = 0; float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (valid) { p = b.val_a[i]; c = b.ctr[p]; }
    const bool left = valid && sah_left(cut, ax, c, i, mid), right = valid && !left;
    const unsigned long long ml = __ballot(left), mr = __ballot(right);
    if (lane_of() == 0u) { wl[wave] = (uint32_t)__popcll(ml); wr[wave] = (uint32_t)__popcll(mr); }
    __syncthreads();
    uint32_t bl = 0, br = 0, tl = 0, tr = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) { if (w < wave) { bl += wl[w]; br += wr[w]; } tl += wl[w]; tr += wr[w]; }
    if (left) { b.val_b[lpos + bl + mbcnt_u64(ml)] = p; bnd_add(lb, c); }
    if (right) { b.val_b[rpos + br + mbcnt_u64(mr)] = p; bnd_add(rb, c); }
    lpos += tl; rpos += tr;
    __syncthreads();
  }
  bnd_wave(lb); bnd_wave(rb);
  if (lane_of() == 0u) {
    uint32_t* cb = b.s_slot[r].cbnd;
    for (int d = 0; d < 3; ++d) {
      if (lb[d] <= lb[3 + d]) { atomicMin(&cb[d], ordered_u(lb[d])); atomicMax(&cb[3 + d], ordered_u(lb[3 + d])); }
      if (rb[d] <= rb[3 + d]) { atomicMin(&cb[6 + d], ordered_u(rb[d])); atomicMax(&cb[9 + d], ordered_u(rb[3 + d])); }
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_sah_big_finish(Bld b, uint32_t level) {
  uint32_t r, first; SahRange e;
  if (!sah_locate(b, level, r, first, e)) return;
  const uint32_t a = e.lo + (blockIdx.x - first) * kSahChunk, z = min(a + kSahChunk - 1u, e.hi);
  for (uint32_t i = a + threadIdx.x; i <= z; i += kBlock) b.val_a[i] = b.val_b[i];
  if (blockIdx.x != first) return;
  SahSlot& s = b.s_slot[r];
  if (threadIdx.x == 0) {
    const uint32_t nblk = (e.hi - e.lo + kSahChunk) / kSahChunk;
    uint32_t nl = 0;
    for (uint32_t k = 0; k < nblk; ++k) nl += b.s_blk[first + k];
    float lb[6], rb[6];
    for (int d = 0; d < 6; ++d) { lb[d] = unordered_f(s.cbnd[d]); rb[d] = unordered_f(s.cbnd[6 + d]); }
    sah_finish(b, e, e.lo + nl - 1u, lb, rb, level);
  }
  __syncthreads();
  for (uint32_t w = threadIdx.x; w < (uint32_t)kBinWords + 12u; w += kBlock) {
    if (w < (uint32_t)kBinWords) s.bins[w] = sah_bin_init(w); else s.cbnd[w - kBinWords] = sah_cbnd_init(w - kBinWords);
  }
}

// ---- bottom-up: box and collapse-cost table of every internal node (ptc_scene.cpp: compute_radix_boxes + "cost tables, bottom-up").  One ROUND per launch: a
// node whose children were complete before this launch computes and stamps itself with the round's number; a child stamped in the same round does not count, so
// everything a node reads was written by an earlier launch and no fence is needed.  (The textbook form — one thread per triangle walks up, the second arrival at
// a node proceeds — needs a release / acquire pair of agent-scope fences per step, and on a chip of 8 XCDs with an L2 each those are L2 write-backs and
// invalidations: 1.6 ms for the 249,936-triangle atrium against 0.4 ms for the ~60 rounds of this one.)
__device__ inline Box link_box(const Bld& b, int32_t link) { return link < 0 ? b.tbox[b.val_a[(size_t)~link]] : b.r_box[(size_t)link]; }
__global__ __launch_bounds__(kBlock) void k_bld_up(Bld b, uint32_t round) {
  const uint32_t cur = blockIdx.x * kBlock + threadIdx.x;
  if (cur + 1u >= b.n || b.r_flag[cur]) return;
  const int32_t left = b.r_left[cur], right = b.r_right[cur];
  if (left >= 0) { const uint32_t f = b.r_flag[left]; if (f == 0u || f >= round) return; }
  if (right >= 0) { const uint32_t f = b.r_flag[right]; if (f == 0u || f >= round) return; }
  {
    const Box bl = link_box(b, left), br = link_box(b, right);
    Box nb = bl;
    grow(nb, br);
    float cl[8], cr[8];
    if (left < 0) dp_row(half_area(bl), cl); else dp_row(b.dp[(size_t)left], cl);
    if (right < 0) dp_row(half_area(br), cr); else dp_row(b.dp[(size_t)right], cr);
    float dist[9];
    const uint32_t kbits = collapse_dist(cl, cr, dist);
    const DpT d = collapse_table(kbits, dist, b.r_hi[cur] - b.r_lo[cur] + 1u, half_area(nb));
    b.r_box[cur] = nb;
    b.dp[cur] = d;
    b.r_flag[cur] = round;
  }
}

// ---- 8-wide collapse, one level of the wide tree per launch (ptc_scene.cpp: expand = forest + make_wide; the decision step and the slots are pt_scene_rules.h's).  A link of a slot: >= 0 the radix node
// of an interior child, kEmptyLink an unused slot, else ~(first sorted position | (triangles - 1) << 28) of a leaf.
struct Kid { int32_t link; bool leaf; uint32_t lo, hi; Box box; };
__device__ inline void forest(const Bld& b, int32_t link0, int i0, Kid* kid, int& n) {
  int32_t sl[16]; int si[16]; int sp = 0;
  sl[sp] = link0; si[sp] = i0; ++sp;
  while (sp > 0) {
    --sp;
    const int32_t link = sl[sp];
    Kid c;
    c.box = link_box(b, link);
    if (link < 0) { c.leaf = true; c.lo = c.hi = (uint32_t)~link; c.link = -1; kid[n++] = c; continue; }
    const uint32_t bits = b.dp[(size_t)link].bits;
    int il, ir;
    if (!forest_split(bits, si[sp], il, ir)) { c.leaf = dp_leaf1(bits); c.lo = b.r_lo[link]; c.hi = b.r_hi[link]; c.link = link; kid[n++] = c; continue; }
    sl[sp] = b.r_right[link]; si[sp] = ir; ++sp;       // left first
    sl[sp] = b.r_left[link]; si[sp] = il; ++sp;
  }
}
__global__ __launch_bounds__(64) void k_bld_widen(Bld b, uint32_t first, uint32_t count) {
  const uint32_t t = blockIdx.x * 64u + threadIdx.x;
  if (t >= count) return;
  const uint32_t idx = first + t;
  const int32_t r = b.w_radix[idx];
  Kid kid[kWide];
  int n = 0;
  {
    const int kk = dp_k(b.dp[(size_t)r].bits, 8);
    forest(b, b.r_left[r], min7(kk), kid, n);
    forest(b, b.r_right[r], min7(8 - kk), kid, n);
  }
  int slot_of[kWide];
  assign_slots(kid, n, slot_of);
  int32_t links[kWide]; uint32_t childs[kWide];
  for (int sl = 0; sl < kWide; ++sl) { links[sl] = (int32_t)kEmptyLink; childs[sl] = kUnset; }
  uint32_t ni = 0, nt = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = slot_of[i];
    if (kid[i].leaf) { links[sl] = (int32_t)leaf_code(kid[i].lo, kid[i].hi - kid[i].lo + 1u); nt += kid[i].hi - kid[i].lo + 1u; }
    else {
      links[sl] = kid[i].link;
      const uint32_t c = atomicAdd(&b.counters[0], 1u);
      b.w_radix[c] = kid[i].link; b.w_parent[c] = idx | ((uint32_t)sl << 28);
      childs[sl] = c; ++ni;
    }
  }
  for (int sl = 0; sl < kWide; ++sl) { b.w_link[(size_t)idx * 8 + sl] = links[sl]; b.w_child[(size_t)idx * 8 + sl] = childs[sl]; }
  b.w_own[idx] = block_units(ni, nt);
  b.w_baddr[idx] = kUnset;
}

// units of a subtree's blocks (its own children block + those of all nodes below), one level per launch from the deepest up
__global__ __launch_bounds__(kBlock) void k_bld_sizes(Bld b, uint32_t first, uint32_t count) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  const uint32_t idx = first + t;
  uint32_t s = b.w_own[idx];
  for (int sl = 0; sl < kWide; ++sl) { const uint32_t c = b.w_child[(size_t)idx * 8 + sl]; if (c != kUnset) s += b.w_sub[c]; }
  b.w_sub[idx] = s;
}

// The top of the layout, by one thread (it is at most `budget` + 7 nodes): children blocks breadth-first while fewer than `budget` nodes are numbered, then every
// numbered node that has no block yet gets the start of its subtree's depth-first stretch (ptc_scene.cpp: alloc_children, "breadth-first top", "depth-first remainder").
__global__ void k_bld_top(Bld b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t* order = b.top_order;
  uint32_t cnt = 1, head = 0, next_unit = 4;
  order[0] = 0u;
  b.w_naddr[0] = 0u;
  for (; head < cnt && cnt < b.budget; ++head) {
    const uint32_t idx = order[head];
    b.w_baddr[idx] = next_unit;
    next_unit += b.w_own[idx];
    for (int sl = 0; sl < kWide; ++sl) { const uint32_t c = b.w_child[(size_t)idx * 8 + sl]; if (c != kUnset) order[cnt++] = c; }
  }
  for (uint32_t i = head; i < cnt; ++i) { const uint32_t idx = order[i]; b.w_baddr[idx] = next_unit; next_unit += b.w_sub[idx]; }
  b.counters[1] = next_unit; b.counters[2] = cnt;
}
// the rest, one level per launch from the root down: a node's block follows its parent's block and the subtrees of its lower interior siblings
__global__ __launch_bounds__(kBlock) void k_bld_addr(Bld b, uint32_t first, uint32_t count) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  const uint32_t idx = first + t;
  const uint32_t pw = b.w_parent[idx];
  if (pw == kUnset) return;                                  // the root
  const uint32_t p = pw & 0x0fffffffu, slot = pw >> 28;
  uint32_t below_units = 0, below_nodes = 0;
  for (uint32_t sl = 0; sl < slot; ++sl) { const uint32_t c = b.w_child[(size_t)p * 8 + sl]; if (c != kUnset) { below_units += b.w_sub[c]; ++below_nodes; } }
  const uint32_t pb = b.w_baddr[p];
  b.w_naddr[idx] = pb + 4u * below_nodes;
  if (b.w_baddr[idx] == kUnset) b.w_baddr[idx] = pb + b.w_own[p] + below_units;
}

// node headers, triangle records (ids only: the refit kernels write the geometry), and the refit's list of node addresses by level
__global__ __launch_bounds__(kBlock) void k_bld_emit(Bld b, uint32_t first, uint32_t count, float4* recs, uint32_t* level_nodes, uint32_t out_first) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  const uint32_t idx = first + t;
  uint32_t imask = 0, lmask = 0, two = 0, ni = 0;
  for (int sl = 0; sl < kWide; ++sl) {
    const uint32_t l = (uint32_t)b.w_link[(size_t)idx * 8 + sl];
    if (l == kEmptyLink) continue;
    if ((int32_t)l >= 0) { imask |= 1u << sl; ++ni; }
    else { lmask |= 1u << sl; if (((~l) >> 28) == 1u) two |= 1u << sl; }
  }
  const uint32_t block = b.w_baddr[idx], at = b.w_naddr[idx];
  const uint32_t none[3] = {0u, 0u, 0u};      // origin, exponents and planes are the refit kernels'
  uint32_t w[3];
  node_header(none, none, node_masks(imask, lmask, two), w);
  reinterpret_cast<uint4*>(recs)[at] = make_uint4(w[0], w[1], w[2], block);
  uint32_t tri = block + 4u * ni;
  for (int sl = 0; sl < kWide; ++sl) {
    if (!((lmask >> sl) & 1u)) continue;
    const uint32_t code = ~(uint32_t)b.w_link[(size_t)idx * 8 + sl];
    const uint32_t lo = code & 0x0fffffffu, cntt = (code >> 28) + 1u;
    for (uint32_t k = 0; k < cntt; ++k) {
      const uint32_t prim = b.val_a[lo + k];
      const float zero[3] = {0.0f, 0.0f, 0.0f};
      tri_record(recs + tri, zero, zero, zero, prim, b.prim_cls[prim]);
      tri += 3u;
    }
  }
  level_nodes[out_first + t] = at;
}

template <class T> T* carve(char*& p, size_t count) {
  T* r = reinterpret_cast<T*>(p);
  p += (count * sizeof(T) + 255u) & ~(size_t)255u;
  return r;
}
#define BLD_TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return std::string("device build: ") + hipGetErrorString(e_); } while (0)
}  // namespace

namespace {
// The front end (sah: the binned-SAH tree, else the LBVH) leaves val_a (sorted position -> primitive id) and r_left / r_right / r_lo / r_hi (internal nodes, the root
// is node 0); the back end from k_bld_up on takes any binary tree over the sorted positions.
std::string build_tree(hipStream_t st, const HostVertex* wverts, const uint32_t* widx, const uint32_t* prim_cls, uint32_t n, uint32_t toplet_budget,
                       BuildScratch& S, BuildOut& out, bool sah) {
  if (n < 2u) return "device build: fewer than two triangles (the host build handles the special case)";
  if (n > (1u << 24)) return "device build: more than 2^24 triangles";
  const uint32_t tiles = (n + kSortTile - 1u) / kSortTile;
  const size_t budget = toplet_budget;
  // ---- scratch: one allocation, carved ----
  Bld b{};
  b.wverts = wverts; b.widx = widx; b.prim_cls = prim_cls; b.n = n; b.budget = toplet_budget;
  auto layout = [&](char* base) {
    char* p = base;
    b.tbox = carve<Box>(p, n); b.cb = carve<uint32_t>(p, 8);
    b.key_a = carve<unsigned long long>(p, n); b.key_b = carve<unsigned long long>(p, n); b.val_a = carve<uint32_t>(p, n); b.val_b = carve<uint32_t>(p, n);
    b.hist = carve<uint32_t>(p, (size_t)(tiles + 4u) * 256u); b.digit_total = carve<uint32_t>(p, 256);
    b.r_left = carve<int32_t>(p, n); b.r_right = carve<int32_t>(p, n); b.r_lo = carve<uint32_t>(p, n); b.r_hi = carve<uint32_t>(p, n);
    b.r_parent = carve<uint32_t>(p, n); b.leaf_parent = carve<uint32_t>(p, n); b.r_flag = carve<uint32_t>(p, n);
    b.r_box = carve<Box>(p, n); b.dp = carve<DpT>(p, n);
    b.w_radix = carve<int32_t>(p, n); b.w_parent = carve<uint32_t>(p, n); b.w_link = carve<int32_t>(p, (size_t)n * 8); b.w_child = carve<uint32_t>(p, (size_t)n * 8);
    b.w_own = carve<uint32_t>(p, n); b.w_sub = carve<uint32_t>(p, n); b.w_baddr = carve<uint32_t>(p, n); b.w_naddr = carve<uint32_t>(p, n);
    b.counters = carve<uint32_t>(p, 8); b.top_order = carve<uint32_t>(p, budget + 16);
    if (sah) {
      b.ctr = carve<float4>(p, n);
      for (int k = 0; k < 2; ++k) { b.s_list[k] = carve<SahRange>(p, n / 2u + 2u); b.s_big[k] = carve<SahRange>(p, n / kSahBig + 2u); }
      b.s_cnt = carve<uint32_t>(p, (size_t)n + 32u); b.s_bigcnt = carve<uint32_t>(p, (size_t)n + 32u);
      b.s_slot = carve<SahSlot>(p, n / kSahBig + 2u); b.s_blk = carve<uint32_t>(p, n / kSahChunk + n / kSahBig + 4u); b.s_root = carve<uint32_t>(p, 2);
    }
    return (size_t)(p - base);
  };
  const size_t need = layout(nullptr);
  if (S.bytes < need) {
    if (S.p) (void)hipFree(S.p);
    S.p = nullptr; S.bytes = 0;
    BLD_TRY(hipMalloc(&S.p, need));
    S.bytes = need;
  }
  layout(static_cast<char*>(S.p));
  const auto blocks = [](uint32_t count, uint32_t per) { return dim3((count + per - 1u) / per); };
  // ---- boxes, keys, sort ----
  hipLaunchKernelGGL(k_bld_init, dim3(1), dim3(64), 0, st, b);
  BLD_TRY(hipMemsetAsync(b.r_flag, 0, (size_t)n * 4, st));
  { uint32_t g = (n + kBlock - 1u) / kBlock; if (g > 1024u) g = 1024u; hipLaunchKernelGGL(k_bld_prims, dim3(g), dim3(kBlock), 0, st, b); }
  if (sah) {
    // ---- the binned-SAH binary tree, top down: levels with big ranges one at a time (the host reads back whether the next level has any), then batches of 16
    // levels of small ranges between read-backs (a level's kernel reads its count from device memory; past the last level the lists are empty) ----
    BLD_TRY(hipMemsetAsync(b.s_cnt, 0, ((size_t)n + 32u) * 4, st));
    BLD_TRY(hipMemsetAsync(b.s_bigcnt, 0, ((size_t)n + 32u) * 4, st));
    BLD_TRY(hipMemsetAsync(b.s_root, 0, 8, st));
    for (void* q : {(void*)b.r_left, (void*)b.r_right, (void*)b.r_hi}) BLD_TRY(hipMemsetAsync(q, 0x7f, (size_t)n * 4, st));
    const uint32_t slots = n / kSahBig + 2u;
    hipLaunchKernelGGL(k_sah_clear, dim3((slots * (uint32_t)(sizeof(SahSlot) / 4u) + kBlock - 1u) / kBlock), dim3(kBlock), 0, st, b, slots);
    hipLaunchKernelGGL(k_sah_init, blocks(n, kBlock), dim3(kBlock), 0, st, b);
    uint32_t gs = (n / 2u + kBlock / 64 - 1u) / (kBlock / 64);
    gs = gs > 2048u ? 2048u : gs;
    const dim3 gsmall(gs), gbig(n / kSahChunk + n / kSahBig + 2u);
    uint32_t level = 0;
    for (uint32_t nbig = n >= kSahBig ? 1u : 0u; nbig;) {
      hipLaunchKernelGGL(k_sah_small, gsmall, dim3(kBlock), 0, st, b, level);
      hipLaunchKernelGGL(k_sah_big_bins, gbig, dim3(kBlock), 0, st, b, level);
      hipLaunchKernelGGL(k_sah_big_count, gbig, dim3(kBlock), 0, st, b, level);
      hipLaunchKernelGGL(k_sah_big_scatter, gbig, dim3(kBlock), 0, st, b, level);
      hipLaunchKernelGGL(k_sah_big_finish, gbig, dim3(kBlock), 0, st, b, level);
      ++level;
      BLD_TRY(hipMemcpyAsync(&nbig, &b.s_bigcnt[level], 4, hipMemcpyDeviceToHost, st));
      BLD_TRY(hipStreamSynchronize(st));
    }
    for (;;) {
      for (int k = 0; k < 16; ++k, ++level) hipLaunchKernelGGL(k_sah_small, gsmall, dim3(kBlock), 0, st, b, level);
      uint32_t open = 0;
      BLD_TRY(hipMemcpyAsync(&open, &b.s_cnt[level], 4, hipMemcpyDeviceToHost, st));
      BLD_TRY(hipStreamSynchronize(st));
      if (!open) break;
      if (level + 16u >= n + 32u) return "device build: the SAH tree is deeper than its triangle count";
    }
    hipLaunchKernelGGL(k_sah_check, blocks(n - 1u, kBlock), dim3(kBlock), 0, st, b);
    uint32_t err = 0;
    BLD_TRY(hipMemcpyAsync(&err, &b.s_root[1], 4, hipMemcpyDeviceToHost, st));
    BLD_TRY(hipStreamSynchronize(st));
    if (err) return "device build: the SAH front end left an inconsistent tree (error bits " + std::to_string(err) + ")";
  } else {
    hipLaunchKernelGGL(k_bld_codes, blocks(n, kBlock), dim3(kBlock), 0, st, b);
    {
      const dim3 g((tiles + kBlock / 64 - 1u) / (kBlock / 64));
      unsigned long long *ki = b.key_a, *ko = b.key_b; uint32_t *vi = b.val_a, *vo = b.val_b;
      for (int pass = 0; pass < 8; ++pass) {          // 63 bits of code: 8 passes of 8; an even number of passes leaves the result in key_a / val_a
        hipLaunchKernelGGL(k_sort_hist, g, dim3(kBlock), 0, st, ki, n, pass * 8, b.hist);
        hipLaunchKernelGGL(k_sort_scan_tiles, dim3(256), dim3(256), 0, st, b.hist, tiles, b.digit_total);
        hipLaunchKernelGGL(k_sort_scan_digits, dim3(1), dim3(256), 0, st, b.digit_total);
        hipLaunchKernelGGL(k_sort_scatter, g, dim3(kBlock), 0, st, ki, vi, n, pass * 8, b.hist, b.digit_total, ko, vo);
        std::swap(ki, ko); std::swap(vi, vo);
      }
    }
    // ---- the radix tree ----
    hipLaunchKernelGGL(k_bld_radix, blocks(n - 1u, kBlock), dim3(kBlock), 0, st, b);
  }
  // ---- boxes, cost tables ----
  for (uint32_t round = 1;;) {            // rounds = the height of the binary tree (40-70 for a scene's Morton codes); the root's stamp is read back every 16
    for (int k = 0; k < 16; ++k, ++round) hipLaunchKernelGGL(k_bld_up, blocks(n - 1u, kBlock), dim3(kBlock), 0, st, b, round);
    uint32_t root_done = 0;
    BLD_TRY(hipMemcpyAsync(&root_done, &b.r_flag[0], 4, hipMemcpyDeviceToHost, st));
    BLD_TRY(hipStreamSynchronize(st));
    if (root_done) break;
    if (round > 8192u && round > n + 16u) return "device build: the binary tree is deeper than 8192 levels";     // (a SAH tree can be as deep as n - 1)
  }
  // ---- 8-wide collapse, level by level ----
  std::vector<uint32_t> lvl_first{0u};
  uint32_t total = 1;
  for (uint32_t first = 0, count = 1; count > 0;) {
    hipLaunchKernelGGL(k_bld_widen, blocks(count, 64), dim3(64), 0, st, b, first, count);
    uint32_t now = 0;
    BLD_TRY(hipMemcpyAsync(&now, &b.counters[0], 4, hipMemcpyDeviceToHost, st));
    BLD_TRY(hipStreamSynchronize(st));
    first += count; count = now - first; total = now;
    lvl_first.push_back(first);
    if (lvl_first.size() > 4096) return "device build: the 8-wide tree is deeper than 4096 levels";
  }
  lvl_first.pop_back();                                      // the last push was the end of the last non-empty level...
  lvl_first.push_back(total);                                // ... which is `total`
  const size_t levels = lvl_first.size() - 1;
  for (size_t l = levels; l-- > 0;) hipLaunchKernelGGL(k_bld_sizes, blocks(lvl_first[l + 1] - lvl_first[l], kBlock), dim3(kBlock), 0, st, b, lvl_first[l], lvl_first[l + 1] - lvl_first[l]);
  hipLaunchKernelGGL(k_bld_top, dim3(1), dim3(64), 0, st, b);
  for (size_t l = 1; l < levels; ++l) hipLaunchKernelGGL(k_bld_addr, blocks(lvl_first[l + 1] - lvl_first[l], kBlock), dim3(kBlock), 0, st, b, lvl_first[l], lvl_first[l + 1] - lvl_first[l]);
  uint32_t ctr[4] = {0, 0, 0, 0};
  BLD_TRY(hipMemcpyAsync(ctr, b.counters, sizeof ctr, hipMemcpyDeviceToHost, st));
  BLD_TRY(hipStreamSynchronize(st));
  const uint32_t n_units = ctr[1];
  if (n_units >= (1u << 31) || n_units < 4u) return "device build: BVH too large";
  // ---- emit ----
  if (!out.recs || out.recs_cap < n_units) {
    if (out.recs) (void)hipFree(out.recs);
    out.recs = nullptr; out.recs_cap = (size_t)n_units + n_units / 8u;
    if (hipMalloc((void**)&out.recs, out.recs_cap * 16) != hipSuccess) { out.recs = nullptr; out.recs_cap = 0; return "device build: out of device memory"; }
  }
  if (!out.level_nodes || out.level_cap < total) {
    if (out.level_nodes) (void)hipFree(out.level_nodes);
    out.level_nodes = nullptr; out.level_cap = (size_t)total + total / 8u;
    if (hipMalloc((void**)&out.level_nodes, out.level_cap * 4) != hipSuccess) { out.level_nodes = nullptr; out.level_cap = 0; return "device build: out of device memory"; }
  }
  float4* recs = out.recs; uint32_t* level_nodes = out.level_nodes;
  BLD_TRY(hipMemsetAsync(recs, 0, (size_t)n_units * 16, st));
  out.level_first.assign(1, 0u);
  uint32_t pos = 0;
  for (size_t l = levels; l-- > 0;) {                        // deepest level first
    const uint32_t count = lvl_first[l + 1] - lvl_first[l];
    hipLaunchKernelGGL(k_bld_emit, blocks(count, kBlock), dim3(kBlock), 0, st, b, lvl_first[l], count, recs, level_nodes, pos);
    pos += count;
    out.level_first.push_back(pos);
  }
  BLD_TRY(hipGetLastError());
  out.n_nodes = total; out.n_units = n_units; out.max_depth = (uint32_t)levels - 1u; out.n_tri_records = n;
  return std::string();
}
}  // namespace

std::string pt_build_lbvh(hipStream_t st, const HostVertex* wverts, const uint32_t* widx, const uint32_t* prim_cls, uint32_t n, uint32_t toplet_budget,
                          BuildScratch& scratch, BuildOut& out) {
  return build_tree(st, wverts, widx, prim_cls, n, toplet_budget, scratch, out, /*sah=*/false);
}
std::string pt_build_sah(hipStream_t st, const HostVertex* wverts, const uint32_t* widx, const uint32_t* prim_cls, uint32_t n, uint32_t toplet_budget,
                         BuildScratch& scratch, BuildOut& out) {
  return build_tree(st, wverts, widx, prim_cls, n, toplet_budget, scratch, out, /*sah=*/true);
}
