// pt_probes.hip — the two kernels of a probe frame (see pt_probes.h; the definition of every value is pt_probe_dir / pt_sh9_basis there, which the host evaluation
// calls too).
//
//   k_raygen_probe    one thread per path, k_raygen's path id -> (probe j = p % n, sample = first + p / n) mapping.  One 16-byte load of the position, four coalesced
//                     16-byte stores: store_primary_ray (pt_pass_common.h).  A streaming kernel like
//                     k_raygen: 64 B written per path, every byte once.
//   k_accumulate_sh   the SH projection of a batch's path radiance.  Every one of a probe's 27 sums runs in sample order with one owner (no atomic: the result does
//                     not depend on how the samples were cut into batches), so only the products L_c b_k are parallel over samples.  A 256-thread block takes 8
//                     probes — one 128-byte line of lpath per sample — and walks the samples 32 at a time.  Phase A, one thread per (probe, sample): load the
//                     16-byte record (the next tile's load is issued first), recompute the path's direction from (base + j, sample) — two hashes, one sincos
//                     polynomial, a square root; the bounces have overwritten the queue by now — and write the 27 products to LDS.  Phase B, one thread per
//                     (probe, sum), 216 of the 256: add the tile's 32 products of its sum in sample order, conflict-free reads.  16 B read per path, the
//                     direction computed once per path, and the serial chain of a sum is one LDS read and one add per sample: a frame of few probes with many
//                     samples, where the first layout tried (a lane per (probe, coefficient) that did load, direction and add per sample in one loop) spent
//                     0.63 us per sample, is bound by that chain alone.
// profiles/probes_atrium.txt has the kernels' times against their byte floors.
#include "pt_probes.h"
#include "pt_pass_common.h"

namespace {
__global__ __launch_bounds__(256) void k_raygen_probe(const float4* __restrict__ pos, uint32_t n_probes, uint32_t base, uint32_t seed_hash, DevQueues q, uint32_t first_sample,
                                                      uint32_t n_paths) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_paths) return;
  const uint32_t j = p % n_probes, sl = p / n_probes;
  const float4 o = pos[j];
  float d[3];
  uint32_t key;
  pt_probe_dir(seed_hash, base + j, first_sample + sl, d, key);
  store_primary_ray(q, p, V3(o.x, o.y, o.z), V3(d), key, true);
}

// tile of k_accumulate_sh: 8 probes (one 128-byte line of lpath per sample) x 32 samples = 256 threads
#define SH_TILE_P 8u
#define SH_TILE_S 32u
__global__ __launch_bounds__(256) void k_accumulate_sh(uint32_t n_probes, uint32_t base, uint32_t seed_hash, const float4* __restrict__ lpath, float* __restrict__ acc,
                                                       uint32_t first_sample, uint32_t n_samples) {
  __shared__ float s_prod[SH_TILE_S * SH_TILE_P * PT_SH9_FLOATS];      // [sample][probe][k][rgb], 27,648 B
  const uint32_t t = threadIdx.x;
  // phase A role: (probe pl, sample sl) of the tile
  const uint32_t pl = t % SH_TILE_P, sl = t / SH_TILE_P;
  const uint32_t j = blockIdx.x * SH_TILE_P + pl;
  const bool probe_ok = j < n_probes;
  // phase B role: the owner of sum m = k * 3 + c of probe ql
  const uint32_t ql = t / (uint32_t)PT_SH9_FLOATS, m = t - ql * (uint32_t)PT_SH9_FLOATS;
  const uint32_t jq = blockIdx.x * SH_TILE_P + ql;
  const bool owner = ql < SH_TILE_P && jq < n_probes;
  float sum = owner ? acc[(size_t)jq * PT_SH9_FLOATS + m] : 0.0f;
  float4 L = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (probe_ok && sl < n_samples) L = lpath[(size_t)sl * n_probes + j];
  for (uint32_t s0 = 0; s0 < n_samples; s0 += SH_TILE_S) {
    const uint32_t s = s0 + sl;
    float4 Ln = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // the next tile's record leaves now and arrives behind this tile's arithmetic
    if (probe_ok && s + SH_TILE_S < n_samples) Ln = lpath[(size_t)(s + SH_TILE_S) * n_probes + j];
    if (probe_ok && s < n_samples) {
      float d[3];
      uint32_t key;
      pt_probe_dir(seed_hash, base + j, first_sample + s, d, key);
      float* o = s_prod + (size_t)t * PT_SH9_FLOATS;      // t = sl * SH_TILE_P + pl
#pragma unroll
      for (int k = 0; k < PT_SH9; ++k) {
        const float b = pt_sh9_basis(k, d[0], d[1], d[2]);
        o[k * 3 + 0] = L.x * b; o[k * 3 + 1] = L.y * b; o[k * 3 + 2] = L.z * b;
      }
    }
    __syncthreads();
    if (owner) {
      const uint32_t cnt = n_samples - s0 < SH_TILE_S ? n_samples - s0 : SH_TILE_S;
      const float* in = s_prod + (size_t)ql * PT_SH9_FLOATS + m;
#pragma unroll 8
      for (uint32_t i = 0; i < cnt; ++i) sum = sum + in[(size_t)i * (SH_TILE_P * PT_SH9_FLOATS)];
    }
    __syncthreads();
    L = Ln;
  }
  if (owner) acc[(size_t)jq * PT_SH9_FLOATS + m] = sum;
}
}  // namespace

void pt_launch_raygen_probe(hipStream_t s, const float4* positions, uint32_t n_probes, uint32_t index_base, uint32_t seed_hash, const DevQueues& q, uint32_t first_sample,
                            uint32_t n_samples) {
  const uint32_t n_paths = n_probes * n_samples;
  if (!n_paths) return;
  const dim3 grid((n_paths + 255u) / 256u);
  hipLaunchKernelGGL(k_raygen_probe, grid, dim3(256), 0, s, positions, n_probes, index_base, seed_hash, q, first_sample, n_paths);
}

void pt_launch_accumulate_sh(hipStream_t s, uint32_t n_probes, uint32_t index_base, uint32_t seed_hash, const float4* lpath, float* acc, uint32_t first_sample, uint32_t n_samples) {
  if (!n_probes || !n_samples) return;
  hipLaunchKernelGGL(k_accumulate_sh, dim3((n_probes + SH_TILE_P - 1u) / SH_TILE_P), dim3(256), 0, s, n_probes, index_base, seed_hash, lpath, acc, first_sample, n_samples);
}
