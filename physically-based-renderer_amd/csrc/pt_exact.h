// pt_exact.h — correctly rounded 1/d, n/d, sqrt(x) and the two-rounding 1/sqrt(x) of normalize3 in fewer instructions than the compiler's expansions.
//
// The arithmetic contract demands IEEE results for / and sqrt, and -fhip-fp32-correctly-rounded-divide-sqrt delivers them: 11 VALU
// instructions per division (2 v_div_scale, v_rcp, 6 fma / mul, v_div_fmas, v_div_fixup, and the VCC hazards between them) and about 14 per square
// root.  Much of that serves operands no shading value has: denormals, huge exponents, zeros, infinities.  The functions here return THE SAME BITS
// from the hardware's 1-ulp seed (v_rcp_f32, v_rsq_f32) and a chain of fused multiply-adds with exact residuals (Markstein, "Computation of
// elementary functions on the IBM RISC System/6000 processor", 1990), behind a guard that keeps every intermediate value normal: no overflow, no
// gradual underflow, no special value.  An operand outside the guard takes the compiler's expansion behind a branch, so every input gets the IEEE
// result.  tests/test_exact_arith_host.py runs the chains under every seed within 1 ulp, exhaustively over the mantissas;
// tests/test_gpu_exact_arith.py holds the device functions to the compiler's / and sqrtf over all 2^32 patterns.
//
// Two parts.  pt_*_ok and pt_*_chain (host + device): the guards and the chains from a given seed, plain IEEE expressions.  pt_rcp, pt_div, pt_div3,
// pt_sqrt, pt_rnorm: what the render arithmetic calls — on the device guard + seed + chain, on the host plain / and sqrtf (overloads on the target, so
// host code and the oracle compute what they always did).  The MODE register is never touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PT_XHD __host__ __device__ __forceinline__
#define PT_XD __device__ __forceinline__

// ---- guards ---------------------------------------------------------------------------------------------------------------------------------
// The window [2^-32, 2^32): exponent field in [95, 159).  With n and d inside it, 1/d lies in (2^-32, 2^32], n/d in (2^-64, 2^64), and a residual of the
// chains is zero or at least 2^-32-47 in magnitude: all normal.  Sixty-four exponents are 2^29 bit patterns, so two operands cost one compare: both
// offsets are below 2^29 iff their OR is.
// A divisor whose mantissa is all ones is the one case the reciprocal chain misses (1/d lies 2^-25 relative above a rounding boundary and the last
// fma of the chain lands ON the boundary when its predecessor is the power of two below): it takes the expansion.
#define PT_X_LO 0x2f800000u       // 2^-32
#define PT_X_SPAN 0x20000000u     // 64 exponents
#define PT_X_MANT 0x007fffffu
PT_XHD uint32_t pt_x_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
PT_XHD uint32_t pt_x_offset(float x) { return (pt_x_bits(x) & 0x7fffffffu) - PT_X_LO; }
PT_XHD bool pt_x_all_ones(float d) { return (~pt_x_bits(d) & PT_X_MANT) == 0u; }
PT_XHD bool pt_rcp_ok(float d) { return pt_x_offset(d) < PT_X_SPAN && !pt_x_all_ones(d); }
PT_XHD bool pt_div_ok(float n, float d) { return (pt_x_offset(n) | pt_x_offset(d)) < PT_X_SPAN && !pt_x_all_ones(d); }
// x > 0 inside the window: the sign bit makes a negative operand's offset huge
PT_XHD bool pt_sqrt_ok(float x) { return pt_x_bits(x) - PT_X_LO < PT_X_SPAN; }
// ... and sqrt(x) does not round to an all-ones mantissa (x within 3 ulp below a power of two), which the reciprocal of the root could not take
PT_XHD bool pt_rnorm_ok(float x) { return pt_sqrt_ok(x) && (~pt_x_bits(x) & (PT_X_MANT - 3u)) != 0u; }
// a numerator of pt_div3, whose divisor lies in [2^-5, 1]: +0, or 2^-32 <= n < 2^96.  (-0 would come out as +0, and is refused with every negative n.)
PT_XHD bool pt_num_ok(float n) { return pt_x_bits(n) - 1u >= PT_X_LO - 1u && pt_x_bits(n) < 0x6f800000u; }   // u - 1 wraps for +0

// ---- chains ---------------------------------------------------------------------------------------------------------------------------------
// r0 within 1 ulp of 1/d -> RN(1/d): two Newton steps with exact residuals
PT_XHD float pt_rcp_chain(float d, float r0) {
  const float e0 = __builtin_fmaf(-d, r0, 1.0f);
  const float r1 = __builtin_fmaf(e0, r0, r0);
  const float e1 = __builtin_fmaf(-d, r1, 1.0f);
  return __builtin_fmaf(e1, r1, r1);
}
// r = RN(1/d) -> RN(n/d): Markstein's correction of the first quotient
PT_XHD float pt_div_chain(float n, float d, float r) {
  const float q = n * r;
  const float rem = __builtin_fmaf(-d, q, n);
  return __builtin_fmaf(rem, r, q);
}
// y0 within 1 ulp of 1/sqrt(x) -> RN(sqrt(x)): one coupled step on s ~ sqrt(x) and h ~ 1/(2 sqrt(x)), then the exact residual x - s^2 times h
PT_XHD float pt_sqrt_chain(float x, float y0) {
  const float h0 = 0.5f * y0;
  const float s0 = x * y0;
  const float r = __builtin_fmaf(-s0, h0, 0.5f);
  const float s1 = __builtin_fmaf(s0, r, s0);
  const float h1 = __builtin_fmaf(h0, r, h0);
  return __builtin_fmaf(__builtin_fmaf(-s1, s1, x), h1, s1);
}
// s = RN(sqrt(x)), y0 as above -> RN(1 / s): y0 is within 2 ulp of 1/s, a seed the reciprocal chain takes as well, so 1/s costs no second transcendental
PT_XHD float pt_rnorm_chain(float s, float y0) { return pt_rcp_chain(s, y0); }

// ---- host: the plain expressions ----------------------------------------------------------------------------------------------------------------
__host__ inline float pt_rcp(float d) { return 1.0f / d; }
__host__ inline float pt_div(float n, float d) { return n / d; }
__host__ inline float pt_sqrt(float x) { return __builtin_sqrtf(x); }
__host__ inline float pt_rnorm(float x, float& s) { s = __builtin_sqrtf(x); return 1.0f / s; }
__host__ inline void pt_div3(float& a, float& b, float& c, float d) { a = a / d; b = b / d; c = c / d; }

// ---- device -------------------------------------------------------------------------------------------------------------------------------------
// The general forms.  Their guard (five fast integer operations, two compares) costs what the expansion spends on its special cases, and at k_shade's general
// divisions they measured SLOWER than the expansion (profiles/shade_exact_arith.txt): those sites keep their plain /.  What pays is what a call site knows:
// one guard for a root and its reciprocal (pt_rnorm), one reciprocal for three numerators over a divisor of known range (pt_div3), a root without a division.
PT_XD float pt_rcp(float d) {
  if (__builtin_expect(pt_rcp_ok(d), 1)) return pt_rcp_chain(d, __builtin_amdgcn_rcpf(d));
  return 1.0f / d;
}
PT_XD float pt_div(float n, float d) {
  if (__builtin_expect(pt_div_ok(n, d), 1)) return pt_div_chain(n, d, pt_rcp_chain(d, __builtin_amdgcn_rcpf(d)));
  return n / d;
}
// three numerators over one divisor that the CALLER knows to lie in [2^-5, 1] (Russian roulette's survival probability): one reciprocal, no window test of d
PT_XD void pt_div3(float& a, float& b, float& c, float d) {
  if (__builtin_expect(pt_num_ok(a) && pt_num_ok(b) && pt_num_ok(c) && !pt_x_all_ones(d), 1)) {
    const float r = pt_rcp_chain(d, __builtin_amdgcn_rcpf(d));
    a = pt_div_chain(a, d, r); b = pt_div_chain(b, d, r); c = pt_div_chain(c, d, r);
    return;
  }
  a = a / d; b = b / d; c = c / d;
}
PT_XD float pt_sqrt(float x) {
  if (__builtin_expect(pt_sqrt_ok(x), 1)) return pt_sqrt_chain(x, __builtin_amdgcn_rsqf(x));
  return __builtin_sqrtf(x);
}
// 1 / sqrt(x) as TWO roundings, s = RN(sqrt(x)) then RN(1 / s): what normalize3 has always computed.  One test of x covers both steps (the root and
// its reciprocal of a window value lie in [2^-16, 2^16]); s is returned as well.
PT_XD float pt_rnorm(float x, float& s) {
  if (__builtin_expect(pt_rnorm_ok(x), 1)) {
    const float y0 = __builtin_amdgcn_rsqf(x);
    s = pt_sqrt_chain(x, y0);
    return pt_rnorm_chain(s, y0);
  }
  s = __builtin_sqrtf(x);
  return 1.0f / s;
}
PT_XHD float pt_rnorm(float x) { float s; return pt_rnorm(x, s); }
