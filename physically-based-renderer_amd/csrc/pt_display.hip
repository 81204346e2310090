// pt_display.hip — metering and display kernels of the display transform (see pt_display.h: every value is defined there, and the host evaluations call the same functions).
//
//   k_meter_hist     256 threads, one pixel (one 16-byte load) per lane and pass, a grid-stride loop over a grid of at most PT_METER_MAX_BLOCKS blocks.  Each block
//                    keeps the 4096-bin histogram in LDS (16 KiB) and adds its non-zero bins to the one in HBM with one no-return atomic each; the rejected
//                    pixels are counted per wave by ballot and added once per wave.  Integer sums only: the result does not depend on any order.
//   k_meter_reduce   one block: thread t owns the 16 bins 16 t .. 16 t + 15.  A block scan gives every bin the rank of its first sample, the trim keeps the ranks in
//                    [n_lo, n_hi), S and M are reduced through LDS, thread 0 forms Q, moves the adaptation state and writes the state record.  The histogram stays.
//   k_display_rgba8  one pixel per thread, templated on operator and transfer function; k_display_half the exposed RGBA16F.  Both compute E from the state record
//                    in HBM, so they are queued behind a metering without the host waiting for it.
// Streaming kernels: metering reads 16 B per pixel, display reads 16 B and writes 4 B (8 B for half) per pixel.
#include "pt_display.h"

#define PT_METER_MAX_BLOCKS 1024u

namespace {
__global__ __launch_bounds__(256) void k_meter_hist(const float4* __restrict__ img, uint32_t n, uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[PT_DISPLAY_BINS];
  for (uint32_t k = threadIdx.x; k < PT_DISPLAY_BINS; k += 256u) bins[k] = 0u;
  __syncthreads();
  const uint32_t stride = gridDim.x * 256u;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t rejected = 0u;      // of this wave: the same value in every lane
  for (uint32_t base = blockIdx.x * 256u; base < n; base += stride) {      // uniform over the block: base < n <= 2^28, stride <= 2^18
    const uint32_t i = base + threadIdx.x;
    int cls = 0;
    uint32_t key = 0u;
    if (i < n) { const float4 c = img[i]; cls = pt_meter_classify(c.x, c.y, c.z, c.w, key); }
    rejected += (uint32_t)__popcll(__ballot(cls == 2));
    if (cls == 1) atomicAdd(&bins[key], 1u);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < PT_DISPLAY_BINS; k += 256u) {
    const uint32_t v = bins[k];
    if (v) atomicAdd(&hist[k], v);
  }
  if (lane == 0u && rejected) atomicAdd(&hist[PT_DISPLAY_BINS], rejected);
}

__global__ __launch_bounds__(256) void k_meter_reduce(const uint32_t* __restrict__ hist, pt_display_state* state, float percentile_lo, float percentile_hi, float adapt_rate) {
  __shared__ uint32_t scan[256];
  __shared__ uint64_t sS[256], sM[256];
  const uint32_t t = threadIdx.x;
  uint32_t cnt[16];
  const uint4* h4 = (const uint4*)hist + t * 4u;
  uint32_t own = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 v = h4[k];
    cnt[4 * k] = v.x; cnt[4 * k + 1] = v.y; cnt[4 * k + 2] = v.z; cnt[4 * k + 3] = v.w;
    own += v.x + v.y + v.z + v.w;
  }
  scan[t] = own;
  __syncthreads();
  for (uint32_t d = 1u; d < 256u; d <<= 1) {      // inclusive scan
    const uint32_t v = t >= d ? scan[t - d] : 0u;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  const uint32_t N = scan[255];
  uint64_t before = (uint64_t)(scan[t] - own);
  uint64_t n_lo, n_hi;
  pt_meter_bounds(N, percentile_lo, percentile_hi, n_lo, n_hi);
  uint64_t S = 0, M = 0;
#pragma unroll
  for (uint32_t k = 0; k < 16u; ++k) {
    const uint64_t kept = pt_meter_kept(before, cnt[k], n_lo, n_hi);
    S += kept * (uint64_t)(2u * (t * 16u + k) + 1u);
    M += kept;
    before += cnt[k];
  }
  sS[t] = S; sM[t] = M;
  __syncthreads();
  for (uint32_t d = 128u; d > 0u; d >>= 1) {
    if (t < d) { sS[t] += sS[t + d]; sM[t] += sM[t + d]; }
    __syncthreads();
  }
  if (t == 0u) {
    const uint64_t St = sS[0], Mt = sM[0];
    const uint32_t Q = pt_meter_mean(St, Mt);
    pt_display_state st;
    st.A = pt_meter_adapt(state->A, Q, Mt, adapt_rate);
    st.Q = Q; st.N = N; st.M = (uint32_t)Mt; st.rejected = hist[PT_DISPLAY_BINS];
    st.pad[0] = st.pad[1] = st.pad[2] = 0u;
    *state = st;
  }
}

template <int OP, int OETF>
__global__ __launch_bounds__(256) void k_display_rgba8(const float4* __restrict__ img, uint32_t n, const pt_display_state* __restrict__ state, ptc_display_params p, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float E = pt_display_scale(p, state->A);
  const float4 c = img[i];
  out[i] = pt_display_pixel8<OP, OETF>(c.x, c.y, c.z, c.w, E, p.white);
}

__global__ __launch_bounds__(256) void k_display_half(const float4* __restrict__ img, uint32_t n, const pt_display_state* __restrict__ state, ptc_display_params p, uint2* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float E = pt_display_scale(p, state->A);
  const float4 c = img[i];
  uint32_t lo, hi;
  pt_display_pixel16(c.x, c.y, c.z, c.w, E, lo, hi);
  out[i] = make_uint2(lo, hi);
}

template <int OP> void launch_rgba8(hipStream_t s, dim3 grid, const float4* img, uint32_t n, const pt_display_state* state, const ptc_display_params& p, uint32_t* out) {
  if (p.oetf == PTC_OETF_SRGB) hipLaunchKernelGGL((k_display_rgba8<OP, PTC_OETF_SRGB>), grid, dim3(256), 0, s, img, n, state, p, out);
  else hipLaunchKernelGGL((k_display_rgba8<OP, PTC_OETF_GAMMA22>), grid, dim3(256), 0, s, img, n, state, p, out);
}
}  // namespace

uint32_t pt_display_meter_grid_pixels() { return PT_METER_MAX_BLOCKS * 256u; }

void pt_launch_meter(hipStream_t s, const float4* img, uint32_t n, uint32_t* hist, pt_display_state* state, const ptc_display_params& p) {
  (void)hipMemsetAsync(hist, 0, (PT_DISPLAY_BINS + 1u) * sizeof(uint32_t), s);
  const uint32_t want = (n + 255u) / 256u;
  const dim3 grid(want < PT_METER_MAX_BLOCKS ? (want ? want : 1u) : PT_METER_MAX_BLOCKS);
  hipLaunchKernelGGL(k_meter_hist, grid, dim3(256), 0, s, img, n, hist);
  hipLaunchKernelGGL(k_meter_reduce, dim3(1), dim3(256), 0, s, hist, state, p.percentile_lo, p.percentile_hi, p.adapt_rate);
}

void pt_launch_display_rgba8(hipStream_t s, const float4* img, uint32_t n, const pt_display_state* state, const ptc_display_params& p, uint32_t* out) {
  if (!n) return;
  const dim3 grid((n + 255u) / 256u);
  switch (p.tonemap) {
    case PTC_TONEMAP_PBR_NEUTRAL: launch_rgba8<PTC_TONEMAP_PBR_NEUTRAL>(s, grid, img, n, state, p, out); break;
    case PTC_TONEMAP_REINHARD: launch_rgba8<PTC_TONEMAP_REINHARD>(s, grid, img, n, state, p, out); break;
    case PTC_TONEMAP_CLAMP: launch_rgba8<PTC_TONEMAP_CLAMP>(s, grid, img, n, state, p, out); break;
    default: launch_rgba8<PTC_TONEMAP_ACES>(s, grid, img, n, state, p, out); break;
  }
}

void pt_launch_display_half(hipStream_t s, const float4* img, uint32_t n, const pt_display_state* state, const ptc_display_params& p, uint2* out) {
  if (!n) return;
  hipLaunchKernelGGL(k_display_half, dim3((n + 255u) / 256u), dim3(256), 0, s, img, n, state, p, out);
}
