// Frame moves of the level schedule of scheduled-sampling training (ss_levels.py): the frames of one
// dependence depth are gathered out of time-major [T][B][W] tensors, run as one forward, and scattered back.
//
// A frame is a slab of L = B * W contiguous floats, so every entry point is a copy of n slabs whose source
// and destination slab are named by device int32 indices:
//   gather       dst[i]      = src[idx[i]]
//   scatter      dst[idx[i]] = src[i]                      (distinct idx: every slab has one writer)
//   level input  dst[i]      = prev[i] >= 0 ? y_prev[prev[i]] : ms[teacher[i]]
// The gradient of the level input with respect to y_prev is the same selection read through the inverse
// map (ms null: the slab is zero), so nothing here adds and no launch needs an atomic.
//
// One launch per call: blockIdx.x is the slab (its indices are wave-uniform scalar loads), blockIdx.y strides
// the slab in pieces of 256 lanes x float4 (one wave per 1 KiB, coalesced).  The float4 form needs W % 4 == 0
// and 16-byte aligned bases (then every slab is aligned too); anything else copies float by float.
#include "mrg_common.h"

namespace mrg {

struct SlabCopy {
  const float* a;     // primary source slabs
  const int* ia;      // slab of a per output (null: i itself); negative: take b
  const float* b;     // secondary source slabs (null: zeros)
  const int* ib;      // slab of b per output
  float* dst;
  const int* id;      // destination slab per output (null: i itself)
  long L;             // floats per slab
};

template <bool VEC>
__global__ __launch_bounds__(256) void slab_copy_kernel(SlabCopy p) {
  const int i = blockIdx.x;
  const float* src = nullptr;
  if (p.ia) {
    const int k = p.ia[i];
    if (k >= 0 && p.a) src = p.a + (long)k * p.L;
    else if (p.b) src = p.b + (long)p.ib[i] * p.L;
  } else {
    src = p.a + (long)i * p.L;
  }
  float* dst = p.dst + (long)(p.id ? p.id[i] : i) * p.L;
  const long first = (long)blockIdx.y * 256 + threadIdx.x, step = (long)gridDim.y * 256;
  if constexpr (VEC) {
    const long n4 = p.L >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (long j = first; j < n4; j += step) d4[j] = src ? s4[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else {
    for (long j = first; j < p.L; j += step) dst[j] = src ? src[j] : 0.0f;
  }
}

static bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

static int slab_copy(const char* who, int n, int B, int W, const SlabCopy& p, hipStream_t stream) {
  const long L = (long)B * W;
  if (n == 0 || L == 0) return 0;
  const bool vec = W % 4 == 0 && aligned16(p.a) && aligned16(p.b) && aligned16(p.dst);
  const long pieces = ((vec ? L / 4 : L) + 255) / 256;
  const dim3 grid((unsigned)n, (unsigned)(pieces < 64 ? pieces : 64));
  if (vec) klaunch(slab_copy_kernel<true>, grid, dim3(256), 0, stream, p);
  else klaunch(slab_copy_kernel<false>, grid, dim3(256), 0, stream, p);
  return check_launch(who);
}

}  // namespace mrg

using namespace mrg;

MRG_API int mrg_frame_gather(int n, int B, int W, const float* src, const int* idx, float* dst, hipStream_t stream) {
  MRG_REQUIRE(n >= 0 && B >= 0 && W >= 0, "mrg_frame_gather: bad sizes (n=%d B=%d W=%d)", n, B, W);
  if (n == 0 || (long)B * W == 0) return 0;
  MRG_REQUIRE(src && idx && dst, "mrg_frame_gather: null buffer");
  SlabCopy p{src, idx, nullptr, nullptr, dst, nullptr, (long)B * W};
  return slab_copy("mrg_frame_gather", n, B, W, p, stream);
}

MRG_API int mrg_frame_scatter(int n, int B, int W, const float* src, const int* idx, float* dst, hipStream_t stream) {
  MRG_REQUIRE(n >= 0 && B >= 0 && W >= 0, "mrg_frame_scatter: bad sizes (n=%d B=%d W=%d)", n, B, W);
  if (n == 0 || (long)B * W == 0) return 0;
  MRG_REQUIRE(src && idx && dst, "mrg_frame_scatter: null buffer");
  SlabCopy p{src, nullptr, nullptr, nullptr, dst, idx, (long)B * W};
  return slab_copy("mrg_frame_scatter", n, B, W, p, stream);
}

MRG_API int mrg_level_input(int n, int B, int W, const float* y_prev, const int* prev, const float* ms,
                            const int* teacher, float* dst, hipStream_t stream) {
  MRG_REQUIRE(n >= 0 && B >= 0 && W >= 0, "mrg_level_input: bad sizes (n=%d B=%d W=%d)", n, B, W);
  if (n == 0 || (long)B * W == 0) return 0;
  MRG_REQUIRE(prev && dst, "mrg_level_input: null buffer");
  MRG_REQUIRE(!ms || teacher, "mrg_level_input: ms without teacher indices");
  SlabCopy p{y_prev, prev, ms, teacher, dst, nullptr, (long)B * W};
  return slab_copy("mrg_level_input", n, B, W, p, stream);
}
