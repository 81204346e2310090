// The fma chains and guards of csrc/pt_exact.h on the host, no GPU: every seed the hardware may return (the correctly rounded reciprocal or reciprocal root
// and its two neighbours: v_rcp_f32 and v_rsq_f32 are accurate to 1 ulp) through the same chains the kernels run, compared with the host's IEEE / and sqrtf.
//   reciprocal       all 2^23 mantissas x 3 seeds x both signs, at the middle and at both edges of the guard's exponent window
//   square root      2^24 operands (both exponent parities) x 3 seeds, likewise; the two-rounding 1/sqrt of normalize3 with them
//   division         10^8 seeded pairs inside the window x 3 seeds, then the hard cases: mantissas of all ones, d = 1 +- ulp, quotients next to a rounding boundary
//   guards           both edges of the window one bit pattern and one exponent either side, zeros, denormals, infinities, NaNs, the all-ones divisors
// Prints "mismatches rcp 0 sqrt 0 rnorm 0 div 0 guard 0" and exits 0 when every result has the reference's bits; tests/test_exact_arith_host.py builds and runs it.
//   hipcc --offload-arch=gfx950 --offload-host-only -std=c++17 -O2 -ffp-contract=off -pthread -Iphysically-based-renderer_amd/csrc tools/exact_arith_host.cpp -o /tmp/exact_arith_host
#include "pt_exact.h"
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t ubits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return ubits(a) == ubits(b); }
static uint64_t mix(uint64_t& s) { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
static std::atomic<long> bad_rcp{0}, bad_sqrt{0}, bad_rnorm{0}, bad_div{0}, bad_guard{0};
static void report(std::atomic<long>& c, const char* what, float a, float b, float seed, float got, float want) {
  if (c.fetch_add(1) < 8) std::printf("%s: a %a (%08x) b %a seed %a: got %a want %a\n", what, a, ubits(a), b, seed, got, want);
}
template <class F> static void parallel(uint64_t n, F f) {
  const unsigned T = 16;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; ++t) th.emplace_back([=] { f(n * t / T, n * (t + 1) / T, t); });
  for (auto& x : th) x.join();
}
// the three seeds within 1 ulp of c
static void seeds3(float c, float s[3]) { s[0] = c; s[1] = std::nextafterf(c, INFINITY); s[2] = std::nextafterf(c, -INFINITY); }

static void expect(bool got, bool want, const char* what, float a, float b) { if (got != want && bad_guard.fetch_add(1) < 8) std::printf("guard %s(%a, %a) = %d, want %d\n", what, a, b, (int)got, (int)want); }
static void check_rcp(float d) {
  if (pt_x_all_ones(d)) { expect(pt_rcp_ok(d), false, "rcp", d, 0); return; }      // the one mantissa the guard sends to the expansion
  const float want = 1.0f / d; float s[3]; seeds3(want, s);
  for (int k = 0; k < 3; ++k) { const float got = pt_rcp_chain(d, s[k]); if (!same(got, want)) report(bad_rcp, "rcp", d, 0, s[k], got, want); }
}
static void check_sqrt(float x) {
  const float want = std::sqrt(x), wantr = 1.0f / want; float s[3]; seeds3((float)(1.0 / std::sqrt((double)x)), s);
  for (int k = 0; k < 3; ++k) {
    const float got = pt_sqrt_chain(x, s[k]);
    if (!same(got, want)) report(bad_sqrt, "sqrt", x, 0, s[k], got, want);
    if (!pt_rnorm_ok(x)) continue;
    const float gr = pt_rnorm_chain(got, s[k]);
    if (!same(gr, wantr)) report(bad_rnorm, "rnorm", x, 0, s[k], gr, wantr);
  }
}
static void check_div(float n, float d) {
  if (pt_x_all_ones(d)) { expect(pt_div_ok(n, d), false, "div", n, d); return; }
  const float want = n / d; float s[3]; seeds3(1.0f / d, s);
  for (int k = 0; k < 3; ++k) { const float got = pt_div_chain(n, d, pt_rcp_chain(d, s[k])); if (!same(got, want)) report(bad_div, "div", n, d, s[k], got, want); }
}

int main() {
  // reciprocal: all 2^23 mantissas, both signs' worth is symmetry (fma is odd in d, r together); exponents at the window's edges as well
  parallel(1u << 23, [](uint64_t a, uint64_t b, unsigned) { for (uint64_t m = a; m < b; ++m) for (uint32_t e : {127u, 95u, 158u}) { check_rcp(bits((e << 23) | (uint32_t)m)); check_rcp(-bits((e << 23) | (uint32_t)m)); } });
  // square root and the two-rounding 1/sqrt: 2^24 operands = both exponent parities, again at the edges too
  parallel(1u << 24, [](uint64_t a, uint64_t b, unsigned) { for (uint64_t m = a; m < b; ++m) for (uint32_t e : {127u, 95u, 157u}) check_sqrt(bits((e << 23) + (uint32_t)m)); });
  // division: 10^8 seeded pairs inside the window
  parallel(100000000ull, [](uint64_t a, uint64_t b, unsigned t) {
    uint64_t s = 0x1234 + t;
    for (uint64_t i = a; i < b; ++i) {
      const uint64_t r = mix(s), r2 = mix(s);
      const uint32_t en = 95u + (uint32_t)(r2 % 64u), ed = 95u + (uint32_t)((r2 >> 8) % 64u);
      check_div(bits(((uint32_t)(r >> 63) << 31) | (en << 23) | ((uint32_t)r & 0x7fffffu)), bits(((uint32_t)(r2 >> 63) << 31) | (ed << 23) | ((uint32_t)(r >> 32) & 0x7fffffu)));
    }
  });
  // hard cases: mantissas of all ones, d = 1 +- ulp, quotients next to a rounding boundary (n = RN(d (q + ulp(q)/2)) and its neighbours)
  parallel(1u << 22, [](uint64_t a, uint64_t b, unsigned t) {
    uint64_t s = 0x9999 + t;
    const float ones = bits(0x3fffffffu), up = bits(0x3f800001u), dn = bits(0x3f7fffffu);
    for (uint64_t i = a; i < b; ++i) {
      const uint64_t r = mix(s);
      const float x = bits(0x3f800000u | ((uint32_t)r & 0x7fffffu)), y = bits(0x3f800000u | ((uint32_t)(r >> 32) & 0x7fffffu));
      check_div(x, ones); check_div(ones, x); check_div(x, up); check_div(x, dn); check_div(up, x); check_div(dn, x);
      const double mid = (double)y + 0.5 * (double)(std::nextafterf(y, 4.0f) - y);
      const float n = (float)((double)x * mid);
      check_div(n, x); check_div(std::nextafterf(n, 8.0f), x); check_div(std::nextafterf(n, 0.0f), x);
    }
  });
  check_div(bits(0x3fffffffu), bits(0x3fffffffu)); check_div(bits(0x3f800001u), bits(0x3f7fffffu)); check_div(bits(0x3f7fffffu), bits(0x3f800001u));
  // a zero numerator of pt_div3
  for (float n : {0.0f}) for (float d : {0.05f, 1.0f, 0.3f}) { const float got = pt_div_chain(n, d, 1.0f / d); if (!same(got, n / d)) report(bad_div, "div0", n, d, 0, got, n / d); }
  // the guards at both edges, one exponent either side, and at the special values
  const float lo = bits(PT_X_LO), below = bits(PT_X_LO - 1u), hi_in = bits(PT_X_LO + PT_X_SPAN - 2u), hi_out = bits(PT_X_LO + PT_X_SPAN);
  for (float sg : {1.0f, -1.0f}) {
    expect(pt_rcp_ok(sg * lo), true, "rcp", lo, 0); expect(pt_rcp_ok(sg * below), false, "rcp", below, 0); expect(pt_rcp_ok(sg * hi_in), true, "rcp", hi_in, 0); expect(pt_rcp_ok(sg * hi_out), false, "rcp", hi_out, 0);
    expect(pt_rcp_ok(sg * lo * 0.5f), false, "rcp", lo * 0.5f, 0); expect(pt_rcp_ok(sg * hi_out * 2.0f), false, "rcp", hi_out * 2.0f, 0);
    for (float o : {lo, hi_in, 1.0f}) {
      expect(pt_div_ok(sg * lo, o), true, "div", lo, o); expect(pt_div_ok(o, sg * lo), true, "div", o, lo); expect(pt_div_ok(sg * hi_in, o), true, "div", hi_in, o); expect(pt_div_ok(o, sg * hi_in), true, "div", o, hi_in);
      expect(pt_div_ok(sg * below, o), false, "div", below, o); expect(pt_div_ok(o, sg * below), false, "div", o, below); expect(pt_div_ok(sg * hi_out, o), false, "div", hi_out, o); expect(pt_div_ok(o, sg * hi_out), false, "div", o, hi_out);
    }
  }
  expect(pt_sqrt_ok(lo), true, "sqrt", lo, 0); expect(pt_sqrt_ok(below), false, "sqrt", below, 0); expect(pt_sqrt_ok(hi_in), true, "sqrt", hi_in, 0); expect(pt_sqrt_ok(hi_out), false, "sqrt", hi_out, 0);
  expect(pt_sqrt_ok(-1.0f), false, "sqrt", -1.0f, 0); expect(pt_sqrt_ok(-lo), false, "sqrt", -lo, 0);
  for (float sp : {0.0f, -0.0f, bits(1u), bits(0x007fffffu), bits(0x00800000u), INFINITY, -INFINITY, NAN, bits(0x7f7fffffu)}) {
    expect(pt_rcp_ok(sp), false, "rcp", sp, 0); expect(pt_sqrt_ok(sp), false, "sqrt", sp, 0); expect(pt_div_ok(sp, 1.0f), false, "div", sp, 1.0f); expect(pt_div_ok(1.0f, sp), false, "div", 1.0f, sp);
  }
  // pt_num_ok: zero passes, the window's lower edge, 2^96 the upper
  expect(pt_num_ok(0.0f), true, "num", 0, 0); expect(pt_num_ok(-0.0f), false, "num", -0.0f, 0); expect(pt_num_ok(bits(1u)), false, "num", bits(1u), 0); expect(pt_num_ok(below), false, "num", below, 0);
  expect(pt_num_ok(lo), true, "num", lo, 0); expect(pt_num_ok(-lo), false, "num", -lo, 0); expect(pt_num_ok(bits(0x6f7fffffu)), true, "num", bits(0x6f7fffffu), 0); expect(pt_num_ok(bits(0x6f800000u)), false, "num", bits(0x6f800000u), 0);
  expect(pt_num_ok(INFINITY), false, "num", INFINITY, 0); expect(pt_num_ok(NAN), false, "num", NAN, 0);
  // all-ones mantissas stay outside, and so do the roots that would round to one
  expect(pt_rcp_ok(bits(0x3fffffffu)), false, "rcp", bits(0x3fffffffu), 0); expect(pt_div_ok(1.0f, bits(0x3fffffffu)), false, "div", 1.0f, bits(0x3fffffffu)); expect(pt_div_ok(bits(0x3fffffffu), 1.5f), true, "div", bits(0x3fffffffu), 1.5f);
  expect(pt_rnorm_ok(bits(0x407ffffeu)), false, "rnorm", bits(0x407ffffeu), 0); expect(pt_rnorm_ok(bits(0x407fffffu)), false, "rnorm", bits(0x407fffffu), 0); expect(pt_rnorm_ok(bits(0x407ffffbu)), true, "rnorm", bits(0x407ffffbu), 0);
  expect(pt_rnorm_ok(lo), true, "rnorm", lo, 0); expect(pt_rnorm_ok(below), false, "rnorm", below, 0); expect(pt_rnorm_ok(bits(PT_X_LO + PT_X_SPAN - 5u)), true, "rnorm", hi_in, 0); expect(pt_rnorm_ok(hi_out), false, "rnorm", hi_out, 0);
  // the extreme quotients of the window: nothing overflows or goes denormal
  for (float n : {lo, hi_in}) for (float d : {lo, hi_in}) { check_div(n, d); check_div(-n, d); }
  // numerators of pt_div3 at their edges over the divisors' edges
  for (float n : {lo, bits(0x6f7fffffu), bits(0x2fffffffu)}) for (float d : {0.03125f, 0.05f, 1.0f, bits(0x3f7fffffu)}) check_div(n, d);
  std::printf("mismatches rcp %ld sqrt %ld rnorm %ld div %ld guard %ld\n", bad_rcp.load(), bad_sqrt.load(), bad_rnorm.load(), bad_div.load(), bad_guard.load());
  return (bad_rcp | bad_sqrt | bad_rnorm | bad_div | bad_guard) ? 1 : 0;
}
