// Dropout on the counter-based RNG of rng.h (gfx950): the draw kernel, the elementwise dropout
// (nn.LSTM / nn.GRU inter-layer dropout, mixer_block.py:169-252) and the keep-mask exports the tests
// compare with the host restatement (rng.py).  Attention-probability dropout lives in attention.hip
// and shares attn_words() with the export below.
#include "mrg_common.h"
#include "rng.h"

namespace mrg {

// key_out = {seed, draw}; draw += 1.  The atomic keeps two streams from taking the same draw.
__global__ void rng_draw_kernel(unsigned long long* state, unsigned long long* key_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long d = atomicAdd(state + 1, 1ull);
    key_out[0] = state[0];
    key_out[1] = d;
  }
}

// thread i owns elements 4 i .. 4 i + 3 (one Philox call): y = keep ? x * scale_keep : 0
__global__ __launch_bounds__(256) void dropout_kernel(long n, uint32_t thr, float scale_keep, int vec,
                                                      const unsigned long long* __restrict__ key,
                                                      const float* __restrict__ x, float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (4 * i >= n) return;
  const Philox4 w = flat_words(load_drop_key(key), (unsigned long long)i);
  if (vec && 4 * i + 3 < n) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x = w.w[0] >= thr ? v.x * scale_keep : 0.0f;
    v.y = w.w[1] >= thr ? v.y * scale_keep : 0.0f;
    v.z = w.w[2] >= thr ? v.z * scale_keep : 0.0f;
    v.w = w.w[3] >= thr ? v.w * scale_keep : 0.0f;
    reinterpret_cast<float4*>(y)[i] = v;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long j = 4 * i + r;
      if (j < n) y[j] = w.w[r] >= thr ? x[j] * scale_keep : 0.0f;
    }
  }
}

__global__ __launch_bounds__(256) void dropout_keep_mask_kernel(long n, uint32_t thr,
                                                                const unsigned long long* __restrict__ key,
                                                                unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (4 * i >= n) return;
  const Philox4 w = flat_words(load_drop_key(key), (unsigned long long)i);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long j = 4 * i + r;
    if (j < n) out[j] = w.w[r] >= thr ? 1 : 0;
  }
}

// grid (ceil(ceil(Tk / 4) / 256), Tq, B * heads): thread -> keys 4 k4 .. 4 k4 + 3 of one (b, head, q)
__global__ __launch_bounds__(256) void attention_keep_mask_kernel(int Tq, int Tk, uint32_t thr,
                                                                  const unsigned long long* __restrict__ key,
                                                                  unsigned char* __restrict__ out) {
  const int k4 = blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y, bh = blockIdx.z;
  if (4 * k4 >= Tk) return;
  const Philox4 w = attn_words(load_drop_key(key), (uint32_t)bh, (uint32_t)q, (uint32_t)k4);
  unsigned char* row = out + ((long)bh * Tq + q) * Tk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = 4 * k4 + r;
    if (k < Tk) row[k] = w.w[r] >= thr ? 1 : 0;
  }
}

}  // namespace mrg

using namespace mrg;

MRG_API int mrg_rng_draw(unsigned long long* state, unsigned long long* key_out, hipStream_t stream) {
  MRG_REQUIRE(state && key_out, "mrg_rng_draw: null buffer");
  MRG_REQUIRE(((((uintptr_t)state | (uintptr_t)key_out)) & 7) == 0, "mrg_rng_draw: buffers must be 8-B aligned");
  rng_draw_kernel<<<1, 1, 0, stream>>>(state, key_out);
  return check_launch("rng_draw_kernel");
}

MRG_API int mrg_dropout(long n, unsigned int thr, float scale_keep, const unsigned long long* key, const float* x,
                        float* y, hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_dropout: n < 0");
  if (n == 0) return 0;
  MRG_REQUIRE(key && x && y, "mrg_dropout: null buffer");
  const long nb = ((n + 3) / 4 + 255) / 256;
  MRG_REQUIRE(nb < (1L << 31), "mrg_dropout: n too large");
  const int vec = ((((uintptr_t)x | (uintptr_t)y) & 15) == 0) ? 1 : 0;
  dropout_kernel<<<(unsigned)nb, 256, 0, stream>>>(n, thr, scale_keep, vec, key, x, y);
  return check_launch("dropout_kernel");
}

MRG_API int mrg_dropout_keep_mask(long n, unsigned int thr, const unsigned long long* key, unsigned char* out,
                                  hipStream_t stream) {
  MRG_REQUIRE(n >= 0, "mrg_dropout_keep_mask: n < 0");
  if (n == 0) return 0;
  MRG_REQUIRE(key && out, "mrg_dropout_keep_mask: null buffer");
  const long nb = ((n + 3) / 4 + 255) / 256;
  MRG_REQUIRE(nb < (1L << 31), "mrg_dropout_keep_mask: n too large");
  dropout_keep_mask_kernel<<<(unsigned)nb, 256, 0, stream>>>(n, thr, key, out);
  return check_launch("dropout_keep_mask_kernel");
}

MRG_API int mrg_attention_keep_mask(int B, int heads, int Tq, int Tk, unsigned int thr,
                                    const unsigned long long* key, unsigned char* out, hipStream_t stream) {
  MRG_REQUIRE(B >= 0 && heads >= 0 && Tq >= 0 && Tk >= 0, "mrg_attention_keep_mask: negative size");
  if (B == 0 || heads == 0 || Tq == 0 || Tk == 0) return 0;
  MRG_REQUIRE(key && out, "mrg_attention_keep_mask: null buffer");
  MRG_REQUIRE(Tq <= 65535 && (long)B * heads <= 65535, "mrg_attention_keep_mask: Tq and B * heads at most 65535");
  dim3 grid(((Tk + 3) / 4 + 255) / 256, Tq, B * heads);
  attention_keep_mask_kernel<<<grid, 256, 0, stream>>>(Tq, Tk, thr, key, out);
  return check_launch("attention_keep_mask_kernel");
}
