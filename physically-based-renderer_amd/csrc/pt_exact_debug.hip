// pt_exact_debug.hip — the kernel behind ptc_debug_exact_arith (include/ptc_exact_debug.h): the fast paths of pt_exact.h against the compiler's correctly
// rounded / and sqrtf, both evaluated on the device under the build's arithmetic flags, bits compared.  Not on the render path.
#include "pt_exact_debug.h"
#include "pt_device.h"

namespace {
PT_DEV float as_f(uint32_t u) { return __builtin_bit_cast(float, u); }
PT_DEV uint32_t as_u(float f) { return __builtin_bit_cast(uint32_t, f); }
PT_DEV bool same(float x, float y) { return as_u(x) == as_u(y) || (x != x && y != y); }
// pattern mode's second operand and the operands of the two-operand ops: seeded hashes of the index; every other index has its exponents moved into
// the fast path's window [2^-32, 2^32), which uniform bit patterns hit only once in sixteen pairs
PT_DEV float hashed(uint32_t i, uint32_t seed, uint32_t salt) {
  uint32_t u = pcg(pcg(i + salt * 0x9e3779b9u) ^ seed);
  if (i & 1u) u = (u & 0x807fffffu) | ((95u + ((u >> 23) & 63u)) << 23);
  return as_f(u);
}

__global__ __launch_bounds__(256) void k_exact_arith(int op, const float* __restrict__ a, const float* __restrict__ b, unsigned long long n, uint32_t first, int cross,
                                                     unsigned long long* __restrict__ out) {
  const unsigned long long total = cross ? n * n : n, stride = (unsigned long long)gridDim.x * 256ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total; i += stride) {
    const bool two = op == PTC_EXACT_DIV || op == PTC_EXACT_DIV3;
    float x, y;
    if (a) { x = a[cross ? i / n : i]; y = b ? b[cross ? i % n : i] : 1.0f; }
    else { x = two ? hashed((uint32_t)i, first, 1u) : as_f(first + (uint32_t)i); y = hashed((uint32_t)i, first, 2u); }
    float got = 0.0f, want = 0.0f;
    bool ok = true;
    if (op == PTC_EXACT_RCP) { got = pt_rcp(x); want = 1.0f / x; ok = same(got, want); }
    else if (op == PTC_EXACT_SQRT) { got = pt_sqrt(x); want = __builtin_sqrtf(x); ok = same(got, want); }
    else if (op == PTC_EXACT_RNORM) {
      float s; got = pt_rnorm(x, s);
      const float ws = __builtin_sqrtf(x); want = 1.0f / ws;
      ok = same(got, want) && same(s, ws);
      if (!same(s, ws)) { got = s; want = ws; }
    } else if (op == PTC_EXACT_DIV) { got = pt_div(x, y); want = x / y; ok = same(got, want); }
    else {   // three numerators (the second is +0 for a quarter of the operands, the third a hash of the first) over a divisor clamped into pt_div3's [2^-5, 1]
      const float d = fmin2(fmax2(__builtin_fabsf(y), 0.03125f), 1.0f);
      float p = x, q = (as_u(y) & 3u) ? as_f(pcg(as_u(x))) : 0.0f, r = as_f(pcg(as_u(x) ^ 0x55555555u));
      const float wp = p / d, wq = q / d, wr = r / d;
      pt_div3(p, q, r, d);
      y = d;
      if (!same(p, wp)) { ok = false; got = p; want = wp; }
      else if (!same(q, wq)) { ok = false; x = as_f(pcg(as_u(x))); got = q; want = wq; }
      else if (!same(r, wr)) { ok = false; x = as_f(pcg(as_u(x) ^ 0x55555555u)); got = r; want = wr; }
    }
    if (!ok) {
      const unsigned long long k = atomicAdd(out, 1ull);
      if (k < PTC_EXACT_OFFENDERS) { out[1 + 4 * k] = as_u(x); out[2 + 4 * k] = as_u(y); out[3 + 4 * k] = as_u(got); out[4 + 4 * k] = as_u(want); }
    }
  }
}
}  // namespace

void pt_launch_exact_arith(hipStream_t s, int op, const float* a, const float* b, unsigned long long n, uint32_t first, int cross, unsigned long long* out) {
  const unsigned long long total = cross ? n * n : n;
  const unsigned long long blocks = (total + 255ull) / 256ull;
  hipLaunchKernelGGL(k_exact_arith, dim3((unsigned)(blocks < 8192ull ? blocks : 8192ull)), dim3(256), 0, s, op, a, b, n, first, cross, out);
}
