// y = a + b over n floats (gfx950): the residual connection without a LayerNorm
// (ResidualConnection(use_layer_norm=False), residual_connection.py:29-37) wherever no GEMM epilogue
// can carry the add (around a recurrence, the one-key attention form).  One pass at HBM rate, 12 bytes
// per element.  The backward needs no kernel: the gradient of y is the gradient of both operands.
#include "mrg_common.h"

namespace mrg {

// thread i owns elements 4 i .. 4 i + 3; y may be a (each element is read before it is written, by
// the thread that writes it), so no __restrict__
__global__ __launch_bounds__(256) void residual_add_kernel(long n, int vec, const float* a, const float* b,
                                                           float* y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (4 * i >= n) return;
  if (vec && 4 * i + 3 < n) {
    const float4 u = reinterpret_cast<const float4*>(a)[i];
    const float4 v = reinterpret_cast<const float4*>(b)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long j = 4 * i + r;
      if (j < n) y[j] = a[j] + b[j];
    }
  }
}

}  // namespace mrg

using namespace mrg;

MRG_API int mrg_residual_add(long n, const float* a, const float* b, float* y, hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_residual_add: n < 0");
  if (n == 0) return 0;
  MRG_REQUIRE(a && b && y, "mrg_residual_add: null buffer");
  const long nb = ((n + 3) / 4 + 255) / 256;
  MRG_REQUIRE(nb < (1L << 31), "mrg_residual_add: n too large");
  const int vec = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) == 0) ? 1 : 0;
  residual_add_kernel<<<(unsigned)nb, 256, 0, stream>>>(n, vec, a, b, y);
  return check_launch("residual_add_kernel");
}
