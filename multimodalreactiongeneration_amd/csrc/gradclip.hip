// Gradient clipping on the flat gradient buffer (Lightning's trainer.gradient_clip_val /
// gradient_clip_algorithm, which the reference sets through Trainer(**cfg.trainer)).
//
// norm   torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type = 2, error_if_nonfinite = False) over
//        one buffer, three launches:
//   partial  256 threads, grid-stride over float4 (at most 1024 blocks), four independent 16-B loads in
//            flight per thread, one fp32 accumulator per load slot, wave_sum, four waves through LDS in a
//            fixed order, one partial per block;
//   final    one block; lane l adds the partials l, l + 256, ... in double, a double butterfly and a
//            fixed-order LDS pass finish the sum; thread 0 writes clip_state = {norm, coef} with
//            coef = min(1, max_norm / (norm + 1e-6f)) in fp32 (a NaN norm gives a NaN coef, as torch);
//   scale    g *= coef in place; coef is read from device memory, and the whole grid returns when
//            coef >= 1 (a multiplication by exactly 1 is the identity, so skipping it is bitwise torch).
//            A NaN coef is not >= 1: it scales, and poisons the gradients as torch does.
// value  torch.clamp(g, -v, v) in place, one launch; a NaN stays NaN.
//
// No floating-point atomics: the order of every addition is a function of (n, alignment) alone, so equal
// inputs give bitwise-equal norms, on one rank or on many.  Nothing about the norm reaches the host: a
// captured step replays the same three launches and clips, or not, by the data of that replay.
// A base pointer that is not 16-byte aligned takes the scalar form of each kernel (same grid).
#include "mrg_common.h"

namespace mrg {

constexpr int GC_MAX_BLOCKS = 1024;   // norm partials (the final kernel reads them from one block)
constexpr int GC_MAP_BLOCKS = 4096;   // the in-place passes, as the optimizer updates

__device__ __forceinline__ float gc_sq(float acc, float v) { return fmaf(v, v, acc); }
__device__ __forceinline__ float gc_sq(float acc, float4 v) {
  return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, acc))));
}

// sum of squares of the m items (float or float4) at p that this thread owns in a grid-stride walk
template <typename T>
__device__ __forceinline__ float gc_sqsum(const T* __restrict__ p, long m) {
  const long S = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (; i + 3 * S < m; i += 4 * S) {
    const T v0 = p[i], v1 = p[i + S], v2 = p[i + 2 * S], v3 = p[i + 3 * S];
    a0 = gc_sq(a0, v0);
    a1 = gc_sq(a1, v1);
    a2 = gc_sq(a2, v2);
    a3 = gc_sq(a3, v3);
  }
  for (; i < m; i += S) a0 = gc_sq(a0, p[i]);
  return (a0 + a1) + (a2 + a3);
}

// part[blockIdx.x] = this block's share of sum g^2.  VEC: g is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void gradclip_sqsum_partial_kernel(const float* __restrict__ g, long n,
                                                                     float* __restrict__ part) {
  float acc;
  if (VEC) {
    const long nv = n >> 2;
    acc = gc_sqsum(reinterpret_cast<const float4*>(g), nv);
    const long t = 4 * nv + (long)blockIdx.x * 256 + threadIdx.x;   // the n % 4 tail
    if (t < n) acc = gc_sq(acc, g[t]);
  } else {
    acc = gc_sqsum(g, n);
  }
  __shared__ float red[4];
  const float w = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void gradclip_final_kernel(const float* __restrict__ part, int nblk,
                                                             float max_norm, float* __restrict__ clip_state) {
  double s = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) s += (double)part[j];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
    const float c = max_norm / (norm + 1e-6f);
    clip_state[0] = norm;
    clip_state[1] = c > 1.0f ? 1.0f : c;   // torch.clamp(c, max = 1): a NaN passes through
  }
}

struct GcScale {
  float c;
  __device__ __forceinline__ float operator()(float v) const { return v * c; }
};
struct GcClamp {
  float v;
  __device__ __forceinline__ float operator()(float x) const { return x < -v ? -v : (x > v ? v : x); }
};

// g[i] = op(g[i]) for i < n, float4 over the aligned body when VEC
template <bool VEC, typename Op>
__device__ __forceinline__ void gc_map(float* __restrict__ g, long n, Op op) {
  const long S = (long)gridDim.x * 256;
  const long t0 = (long)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const long nv = n >> 2;
    float4* g4 = reinterpret_cast<float4*>(g);
    for (long i = t0; i < nv; i += S) {
      float4 v = g4[i];
      v.x = op(v.x); v.y = op(v.y); v.z = op(v.z); v.w = op(v.w);
      g4[i] = v;
    }
    const long t = 4 * nv + t0;
    if (t < n) g[t] = op(g[t]);
  } else {
    for (long i = t0; i < n; i += S) g[i] = op(g[i]);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gradclip_scale_kernel(float* __restrict__ g, long n,
                                                             const float* __restrict__ clip_state) {
  const float c = clip_state[1];
  if (c >= 1.0f) return;   // uniform: this step does not clip
  gc_map<VEC>(g, n, GcScale{c});
}

template <bool VEC>
__global__ __launch_bounds__(256) void gradclip_value_kernel(float* __restrict__ g, long n, float v) {
  gc_map<VEC>(g, n, GcClamp{v});
}

// ------------------------------------------------------------------ under gradient accumulation
// Lightning's accumulate_grad_batches = n (the accum kernels of norm_loss_optim.hip): g holds the SUM of
// the window's micro-batch gradients and accum = device int[2] {micro, n}.  Every launch below returns
// after reading those 8 bytes unless this call closes the window (micro + 1 >= n), so off the boundary g
// and clip_state keep their bits.  On the boundary they clip the MEAN g / n without a pass of its own:
//   partial  as above, over the sum (same reads, same order of additions);
//   final    norm = sqrt(sum g^2) / n in double, then the coefficient as above from that norm;
//   scale    g *= coef / n when coef < 1 (or NaN), else nothing: a step that does not clip leaves the
//            division to the update kernel, which reads the same coefficient and decides the same way;
//   value    g = clamp(g / n, -v, v), always; the update kernel is told so (prescaled).
__device__ __forceinline__ bool gc_off_boundary(const int* __restrict__ accum) {
  return accum[0] + 1 < accum[1];
}

template <bool VEC>
__global__ __launch_bounds__(256) void gradclip_sqsum_partial_accum_kernel(const float* __restrict__ g, long n,
                                                                           float* __restrict__ part,
                                                                           const int* __restrict__ accum) {
  if (gc_off_boundary(accum)) return;   // uniform
  float acc;
  if (VEC) {
    const long nv = n >> 2;
    acc = gc_sqsum(reinterpret_cast<const float4*>(g), nv);
    const long t = 4 * nv + (long)blockIdx.x * 256 + threadIdx.x;   // the n % 4 tail
    if (t < n) acc = gc_sq(acc, g[t]);
  } else {
    acc = gc_sqsum(g, n);
  }
  __shared__ float red[4];
  const float w = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void gradclip_final_accum_kernel(const float* __restrict__ part, int nblk,
                                                                   float max_norm, float* __restrict__ clip_state,
                                                                   const int* __restrict__ accum) {
  if (gc_off_boundary(accum)) return;   // uniform
  double s = 0.0;
  for (int j = threadIdx.x; j < nblk; j += 256) s += (double)part[j];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float norm = (float)(sqrt((red[0] + red[1]) + (red[2] + red[3])) / (double)accum[1]);
    const float c = max_norm / (norm + 1e-6f);
    clip_state[0] = norm;
    clip_state[1] = c > 1.0f ? 1.0f : c;
  }
}

struct GcMeanClamp {
  float s, v;
  __device__ __forceinline__ float operator()(float x) const {
    x *= s;
    return x < -v ? -v : (x > v ? v : x);
  }
};

template <bool VEC>
__global__ __launch_bounds__(256) void gradclip_scale_accum_kernel(float* __restrict__ g, long n,
                                                                   const float* __restrict__ clip_state,
                                                                   const int* __restrict__ accum) {
  if (gc_off_boundary(accum)) return;
  const float c = clip_state[1];
  if (c >= 1.0f) return;   // uniform: this window does not clip, the update divides by n
  gc_map<VEC>(g, n, GcScale{c * (1.0f / (float)accum[1])});
}

template <bool VEC>
__global__ __launch_bounds__(256) void gradclip_value_accum_kernel(float* __restrict__ g, long n, float v,
                                                                   const int* __restrict__ accum) {
  if (gc_off_boundary(accum)) return;
  gc_map<VEC>(g, n, GcMeanClamp{1.0f / (float)accum[1], v});
}

static int gc_blocks(long n, int cap) {
  const long b = ((n + 3) / 4 + 255) / 256;   // one float4 per thread per sweep
  return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

static bool gc_aligned(const float* g) { return ((uintptr_t)g & 15) == 0; }

}  // namespace mrg

using namespace mrg;

MRG_API size_t mrg_grad_clip_workspace_bytes(long n) {
  return (size_t)gc_blocks(n < 0 ? 0 : n, GC_MAX_BLOCKS) * sizeof(float);
}

// clip_state: device float[2] = {total norm before clipping, coefficient applied}, overwritten.
MRG_API int mrg_grad_clip_norm(float* grads, long n, float max_norm, float* clip_state, void* ws,
                               hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_grad_clip_norm: n = %ld", n);
  MRG_REQUIRE(max_norm >= 0.0f, "mrg_grad_clip_norm: max_norm %g (must be >= 0, not NaN)", (double)max_norm);
  if (n == 0) return 0;
  MRG_REQUIRE(grads && clip_state && ws, "mrg_grad_clip_norm: null pointer");
  float* part = reinterpret_cast<float*>(ws);
  const int nb = gc_blocks(n, GC_MAX_BLOCKS), mb = gc_blocks(n, GC_MAP_BLOCKS);
  const bool vec = gc_aligned(grads);
  if (vec)
    gradclip_sqsum_partial_kernel<true><<<nb, 256, 0, stream>>>(grads, n, part);
  else
    gradclip_sqsum_partial_kernel<false><<<nb, 256, 0, stream>>>(grads, n, part);
  if (check_launch("gradclip_sqsum_partial_kernel")) return 1;
  gradclip_final_kernel<<<1, 256, 0, stream>>>(part, nb, max_norm, clip_state);
  if (check_launch("gradclip_final_kernel")) return 1;
  if (vec)
    gradclip_scale_kernel<true><<<mb, 256, 0, stream>>>(grads, n, clip_state);
  else
    gradclip_scale_kernel<false><<<mb, 256, 0, stream>>>(grads, n, clip_state);
  return check_launch("gradclip_scale_kernel");
}

MRG_API int mrg_grad_clip_value(float* grads, long n, float clip_value, hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_grad_clip_value: n = %ld", n);
  MRG_REQUIRE(clip_value >= 0.0f, "mrg_grad_clip_value: clip_value %g (must be >= 0, not NaN)",
              (double)clip_value);
  if (n == 0) return 0;
  MRG_REQUIRE(grads, "mrg_grad_clip_value: null pointer");
  const int mb = gc_blocks(n, GC_MAP_BLOCKS);
  if (gc_aligned(grads))
    gradclip_value_kernel<true><<<mb, 256, 0, stream>>>(grads, n, clip_value);
  else
    gradclip_value_kernel<false><<<mb, 256, 0, stream>>>(grads, n, clip_value);
  return check_launch("gradclip_value_kernel");
}

// The two above for a window of accumulated gradients (see "under gradient accumulation").  accum: device
// int[2] = {micro, n}, read only.  Same grids as the plain entry points, on and off the boundary.
MRG_API int mrg_grad_clip_norm_accum(float* grads, long n, float max_norm, float* clip_state, void* ws,
                                     const int* accum, hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_grad_clip_norm_accum: n = %ld", n);
  MRG_REQUIRE(max_norm >= 0.0f, "mrg_grad_clip_norm_accum: max_norm %g (must be >= 0, not NaN)",
              (double)max_norm);
  if (n == 0) return 0;
  MRG_REQUIRE(grads && clip_state && ws && accum, "mrg_grad_clip_norm_accum: null pointer");
  float* part = reinterpret_cast<float*>(ws);
  const int nb = gc_blocks(n, GC_MAX_BLOCKS), mb = gc_blocks(n, GC_MAP_BLOCKS);
  const bool vec = gc_aligned(grads);
  if (vec)
    gradclip_sqsum_partial_accum_kernel<true><<<nb, 256, 0, stream>>>(grads, n, part, accum);
  else
    gradclip_sqsum_partial_accum_kernel<false><<<nb, 256, 0, stream>>>(grads, n, part, accum);
  if (check_launch("gradclip_sqsum_partial_accum_kernel")) return 1;
  gradclip_final_accum_kernel<<<1, 256, 0, stream>>>(part, nb, max_norm, clip_state, accum);
  if (check_launch("gradclip_final_accum_kernel")) return 1;
  if (vec)
    gradclip_scale_accum_kernel<true><<<mb, 256, 0, stream>>>(grads, n, clip_state, accum);
  else
    gradclip_scale_accum_kernel<false><<<mb, 256, 0, stream>>>(grads, n, clip_state, accum);
  return check_launch("gradclip_scale_accum_kernel");
}

MRG_API int mrg_grad_clip_value_accum(float* grads, long n, float clip_value, const int* accum,
                                      hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_grad_clip_value_accum: n = %ld", n);
  MRG_REQUIRE(clip_value >= 0.0f, "mrg_grad_clip_value_accum: clip_value %g (must be >= 0, not NaN)",
              (double)clip_value);
  if (n == 0) return 0;
  MRG_REQUIRE(grads && accum, "mrg_grad_clip_value_accum: null pointer");
  const int mb = gc_blocks(n, GC_MAP_BLOCKS);
  if (gc_aligned(grads))
    gradclip_value_accum_kernel<true><<<mb, 256, 0, stream>>>(grads, n, clip_value, accum);
  else
    gradclip_value_accum_kernel<false><<<mb, 256, 0, stream>>>(grads, n, clip_value, accum);
  return check_launch("gradclip_value_accum_kernel");
}
