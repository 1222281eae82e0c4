// Elementwise activations (gfx950) for the places where an activation is not followed by a Linear
// of the same autograd function, so no GEMM epilogue can carry it: the attention output
// nonlinearity of MHAforSequentail (for_sequential.py:47-51) and the last resort of the
// feed-forward dispatch.  kind 1 relu, 2 tanh, 3 silu.  Forward y = act(x); backward
// dx = dy * act'(saved), saved = the post-activation for relu and tanh, the pre-activation for silu
// (z sigma(z) is not invertible).  Same transcendentals as the GEMM epilogues 4..7 (gemm_common.h).
#include "mrg_common.h"

namespace mrg {

__device__ __forceinline__ float act_fwd(int kind, float x) {
  if (kind == 1) return fmaxf(x, 0.0f);
  if (kind == 2) return tanhf_(x);
  return x * sigmoidf_(x);
}

__device__ __forceinline__ float act_bwd(int kind, float dy, float s) {
  if (kind == 1) return s > 0.0f ? dy : 0.0f;
  if (kind == 2) return dy * (1.0f - s * s);
  const float g = sigmoidf_(s);
  return dy * (g * (1.0f + s * (1.0f - g)));
}

// thread i owns elements 4 i .. 4 i + 3: one 16-B access per operand when vec (every base pointer
// 16-B aligned) and the four are inside n, element-wise otherwise
__global__ __launch_bounds__(256) void activation_fwd_kernel(long n, int kind, int vec, const float* __restrict__ x,
                                                             float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (vec && 4 * i + 3 < n) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x = act_fwd(kind, v.x); v.y = act_fwd(kind, v.y); v.z = act_fwd(kind, v.z); v.w = act_fwd(kind, v.w);
    reinterpret_cast<float4*>(y)[i] = v;
  } else {
    for (long j = 4 * i; j < n && j < 4 * i + 4; ++j) y[j] = act_fwd(kind, x[j]);
  }
}

__global__ __launch_bounds__(256) void activation_bwd_kernel(long n, int kind, int vec, const float* __restrict__ dy,
                                                             const float* __restrict__ saved,
                                                             float* __restrict__ dx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (vec && 4 * i + 3 < n) {
    const float4 g = reinterpret_cast<const float4*>(dy)[i];
    const float4 s = reinterpret_cast<const float4*>(saved)[i];
    float4 v;
    v.x = act_bwd(kind, g.x, s.x); v.y = act_bwd(kind, g.y, s.y);
    v.z = act_bwd(kind, g.z, s.z); v.w = act_bwd(kind, g.w, s.w);
    reinterpret_cast<float4*>(dx)[i] = v;
  } else {
    for (long j = 4 * i; j < n && j < 4 * i + 4; ++j) dx[j] = act_bwd(kind, dy[j], saved[j]);
  }
}

}  // namespace mrg

using namespace mrg;

MRG_API int mrg_activation_fwd(long n, int kind, const float* x, float* y, hipStream_t stream) {
  MRG_REQUIRE(n >= 0 && kind >= 1 && kind <= 3, "mrg_activation_fwd: bad kind %d (1 relu, 2 tanh, 3 silu)", kind);
  if (n == 0) return 0;
  MRG_REQUIRE(x && y, "mrg_activation_fwd: null buffer");
  const long nb = ((n + 3) / 4 + 255) / 256;
  MRG_REQUIRE(nb < (1L << 31), "mrg_activation_fwd: n too large");
  const int vec = ((((uintptr_t)x | (uintptr_t)y) & 15) == 0) ? 1 : 0;
  activation_fwd_kernel<<<(unsigned)nb, 256, 0, stream>>>(n, kind, vec, x, y);
  return check_launch("activation_fwd_kernel");
}

MRG_API int mrg_activation_bwd(long n, int kind, const float* dy, const float* saved, float* dx,
                               hipStream_t stream) {
  MRG_REQUIRE(n >= 0 && kind >= 1 && kind <= 3, "mrg_activation_bwd: bad kind %d (1 relu, 2 tanh, 3 silu)", kind);
  if (n == 0) return 0;
  MRG_REQUIRE(dy && saved && dx, "mrg_activation_bwd: null buffer");
  const long nb = ((n + 3) / 4 + 255) / 256;
  MRG_REQUIRE(nb < (1L << 31), "mrg_activation_bwd: n too large");
  const int vec = ((((uintptr_t)dy | (uintptr_t)saved | (uintptr_t)dx) & 15) == 0) ? 1 : 0;
  activation_bwd_kernel<<<(unsigned)nb, 256, 0, stream>>>(n, kind, vec, dy, saved, dx);
  return check_launch("activation_bwd_kernel");
}
