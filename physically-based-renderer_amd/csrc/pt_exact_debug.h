// pt_exact_debug.h — the launcher of ptc_debug_exact_arith's kernel (pt_exact_debug.hip), for ptc_api_debug.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ptc.h"

// out: 1 + 4 * PTC_EXACT_OFFENDERS words in device memory, zeroed by the caller; a, b: device arrays or null (include/ptc_exact_debug.h has the modes)
void pt_launch_exact_arith(hipStream_t, int op, const float* a, const float* b, unsigned long long n, uint32_t first, int cross, unsigned long long* out);
