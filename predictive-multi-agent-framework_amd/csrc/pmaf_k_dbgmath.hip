// pmaf_k_dbgmath.hip -- k_debug_math_ext, the kernel behind ops 13..20 of pmaf_debug_math (include/pmaf.h), and its
// launcher. Test support only: the elementary operations of the arithmetic policies (pmaf_device.hpp) that ops 0..12
// (k_debug_math, pmaf_k_misc.hip) do not reach -- the default policy's select-free square root and its refined reciprocal by itself, the
// opt-in fast policy's reciprocal, root and shared reciprocal root -- evaluated one element per thread so that
// tests/test_hard_rounding_gpu.py and tests/test_rcp_bias_gpu.py can hold them to constructed hard-to-round operands. A translation unit of its own,
// like pmaf_k_slack.hip: the code objects of the other units stay byte for byte what they were.
#include <hip/hip_runtime.h>

#include "pmaf_types.hpp"
#include "pmaf_device.hpp"

using namespace pmaf;

__global__ void k_debug_math_ext(int op, int n, const double *a, const double *b, double *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r = 0.0;
  switch (op) {
    case 13: r = Mth<MATH_XACT>::sqrt_pos(a[i]); break;
    case 14: r = Mth<MATH_FAST>::div(a[i], b[i]); break;
    case 15: r = Mth<MATH_FAST>::sqrt(a[i]); break;
    case 16: { double s, y; Mth<MATH_FAST>::sqrt_rsqrt(b[i], s, y); r = y; } break;                                   // ~ 1 / sqrt(b)
    case 17: { double s, y; Mth<MATH_FAST>::sqrt_rsqrt(b[i], s, y); r = Mth<MATH_FAST>::div_n(a[i], s, y); } break;  // ~ a / sqrt(b)
    case 18: r = Mth<MATH_XACT>::rcp_refined(b[i]); break;                                                           // RN(1 / b)
    case 19: { double s, rs; Mth<MATH_XACT>::norm_rcp_z(b[i], s, rs); r = rs; } break;                               // RN(1 / sqrt(b)'s double), root's seed
    case 20: { double s, rs; Mth<MATH_XACT>::norm_rcp_zpos(b[i], s, rs); r = Mth<MATH_XACT>::div_r_pos(a[i], s, rs); } break;  // a / sqrt(b)
  }
  out[i] = r;
}

void pmaf_k_launch_debug_math_ext(int op, int n, const double *a, const double *b, double *out, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_math_ext, dim3((n + 255) / 256), dim3(256), 0, s, op, n, a, b, out);
}
