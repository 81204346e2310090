/* ptc_exact_debug.h - test hook for the exact fast paths of division and square root (csrc/pt_exact.h, DESIGN.md "Arithmetic contract").
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface like ptc_shade_debug.h, which it follows: in C and C++ the function has the name below; libptc.so exports it as
 * ptcx_<name without its ptc_>, which the macro maps.  A binding that looks symbols up by name (dlsym, ctypes) asks for the ptcx_ name. */
#ifndef PTC_EXACT_DEBUG_H
#define PTC_EXACT_DEBUG_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_debug_exact_arith ptcx_debug_exact_arith

#define PTC_EXACT_RCP 0       /* pt_rcp(a)            against 1.0f / a                        */
#define PTC_EXACT_SQRT 1      /* pt_sqrt(a)           against sqrtf(a)                        */
#define PTC_EXACT_RNORM 2     /* pt_rnorm(a, s)       against s = sqrtf(a), 1.0f / s (both)   */
#define PTC_EXACT_DIV 3       /* pt_div(a, b)         against a / b                           */
#define PTC_EXACT_DIV3 4      /* pt_div3(a, a', a'', b) against a / b, with b clamped into [2^-5, 1] as the caller's contract demands */
#define PTC_EXACT_OFFENDERS 16

#ifdef __cplusplus
extern "C" {
#endif

/* Test hook.  Evaluates fast path `op` and the compiler's correctly rounded / or sqrtf ON THE DEVICE of the context and compares the bits (NaNs compare equal
 * to NaNs).  Operands:
 *   a == NULL, b == NULL: pattern mode.  Operand i of n is the bit pattern first + i (32-bit wrap); for the two-operand ops the second operand is a seeded
 *     hash of i (and `first` seeds it), so n = 2^32 covers every pattern of the first operand.
 *   a != NULL: n explicit operands a[i]; b[i] the second operand of the two-operand ops (b may be NULL for the others).
 *   cross != 0 (explicit mode, two-operand ops): the full cross product a[i] op b[j], i < n, j < n, instead of the pairs.
 * out[0] = number of mismatches; out[1 + 4 k .. 4 + 4 k], k < min(out[0], 16): the bits of a, of b, of the fast path's result and of the reference's, for the
 * first mismatches found (in no particular order).  out has 1 + 4 * PTC_EXACT_OFFENDERS words.
 * PTC_E_ARG: a null context or out, an unknown op, n = 0 (n is 64-bit: 2^32 is a count), b without a, cross in pattern mode or with more than 2^16 operands. */
int ptc_debug_exact_arith(ptc_ctx*, int op, const float* a, const float* b, uint64_t n, uint32_t first, int cross, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* PTC_EXACT_DEBUG_H */
