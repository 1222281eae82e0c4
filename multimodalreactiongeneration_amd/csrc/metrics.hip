// Per-target MSE metrics (mr_gen/utils/metrics/multi_modal_metrics.py:6-56): one squared-error mean per
// column range [start_k, end_k) of the pose vector, accumulated over update() calls in device memory.
//
// Per element the term is the `type = mse` term of the loss kernels (norm_loss_optim.hip loss_elem /
// bcast_elem, restated here with the loss type fixed): l = d * d, added into every range k with
// start_k <= f < end_k (ranges may overlap).  An update is two launches:
//   partial  256 threads, grid-stride, K fp32 register accumulators per thread, wave_sum, four waves through
//            LDS, one row of K partials per block;
//   final    one block; wave w sums the block partials of range k = w, w + 4 in a fixed order in double and
//            advances state[k] = {sum, count} (double [K][2]) and batch_out[k] = sum / count_k.
// No floating-point atomics: the order of every addition is a function of the launch shape alone, so two
// identical runs leave bitwise-equal state.  The state lives in device memory and is advanced by the kernel
// (as the AdamW step counter and the dropout RNG state are), so a replayed HIP graph keeps accumulating.
// count_k is a launch constant: padded positions count, as in the reference (mask, then mean over all).
#include "mrg_common.h"

namespace mrg {

constexpr int MET_MAXK = 8;

struct MetRanges {
  int K;
  int start[MET_MAXK];
  int end[MET_MAXK];
};

// y viewed [B, T, F] with batch stride ys (y[:, lead:] slices), target contiguous [B, T, F]
struct MetPlain {
  const float* y;
  long ys;
  const float* t;
  int B, T, F;
  int mask_padding;
  int delta_start;
  float dscale;  // sqrt(delta_loss_scale) for features >= delta_start

  __device__ __forceinline__ float operator()(long i, int f) const {
    const long bt = i / F;
    const int b = bt / T, tt = bt % T;
    const float yv = y[(long)b * ys + (long)tt * F + f];
    const float tv = t[i];
    const float m = (mask_padding && tv == -100.0f) ? 0.0f : 1.0f;
    const float s = f >= delta_start ? dscale : 1.0f;
    const float d = (yv * m) * s - (tv * m) * s;
    return d * d;
  }
};

// The broadcast [Tm, B, T, F] target of the generation paths, collapsed as in bcast_elem:
// with c1 = #{t' : ms[b, t', f] != -100}, c0 = Tm - c1,
//   sum_t' l = c1 * (target pad ? 0 : (s y - s t)^2) + c0 * (s y)^2
struct MetBcast {
  const float* y;
  long ys;
  const float* t;
  const float* counts;  // [B * F] = c1
  int B, T, F, Tm;
  int t_start;  // scaler applies to time index t >= t_start
  float dscale;

  __device__ __forceinline__ float operator()(long i, int f) const {
    const long bt = i / F;
    const int b = bt / T, tt = bt % T;
    const float yv = y[(long)b * ys + (long)tt * F + f];
    const float tv = t[i];
    const float c1 = counts[b * F + f];
    const float c0 = (float)Tm - c1;
    const float s = tt >= t_start ? dscale : 1.0f;
    float l1 = 0.0f;
    if (tv != -100.0f) {
      const float d = yv * s - tv * s;
      l1 = d * d;
    }
    const float d0 = yv * s;
    return c1 * l1 + c0 * (d0 * d0);
  }
};

__global__ __launch_bounds__(256) void met_count_kernel(const float* __restrict__ ms, long ms_bs, long ms_ts,
                                                        int B, int Tm, int F, float* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * F) return;
  const int b = i / F, f = i % F;
  const float* p = ms + (long)b * ms_bs + f;
  int c = 0;
  for (int t = 0; t < Tm; ++t) c += p[(long)t * ms_ts] != -100.0f;
  counts[i] = (float)c;
}

// part[blockIdx.x][K]
template <typename Elem>
__global__ __launch_bounds__(256) void met_partial_kernel(Elem a, MetRanges r, float* __restrict__ part) {
  const long n = (long)a.B * a.T * a.F;
  float acc[MET_MAXK];
#pragma unroll
  for (int k = 0; k < MET_MAXK; ++k) acc[k] = 0.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int f = i % a.F;
    const float l = a(i, f);
#pragma unroll
    for (int k = 0; k < MET_MAXK; ++k)
      if (k < r.K && f >= r.start[k] && f < r.end[k]) acc[k] += l;
  }
  __shared__ float red[4][MET_MAXK];
#pragma unroll
  for (int k = 0; k < MET_MAXK; ++k) {
    const float v = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < r.K) {
    const int k = threadIdx.x;
    part[(long)blockIdx.x * r.K + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

struct MetCounts {
  double n[MET_MAXK];
};

// One block of four waves; wave w owns ranges k = w, w + 4.  Lane j adds partials j, j + 64, ... in double,
// then a butterfly over the 64 lanes (a + b == b + a bitwise, so every lane holds the same sum).
__global__ __launch_bounds__(256) void met_final_kernel(const float* __restrict__ part, int nblk, int K,
                                                        MetCounts cnt, double* __restrict__ state,
                                                        float* __restrict__ batch_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int kk = 0; kk < MET_MAXK / 4; ++kk) {
    const int k = __builtin_amdgcn_readfirstlane(wave + 4 * kk);   // wave-uniform: cnt.n[k] is a scalar load
    if (k >= K) break;
    double s = 0.0;
    for (int j = lane; j < nblk; j += 64) s += (double)part[(long)j * K + k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
      const double c = cnt.n[k];
      state[2 * k] += s;
      state[2 * k + 1] += c;
      batch_out[k] = (float)(s / c);
    }
  }
}

static int met_blocks(long n) {
  long b = (n + 255) / 256;
  return (int)(b < 1024 ? (b < 1 ? 1 : b) : 1024);
}

// Ranges by value into the launch struct; counts per range = rows * (end - start).
static int met_ranges(const char* who, int F, int K, const int* starts, const int* ends, double rows,
                      MetRanges& r, MetCounts& c) {
  MRG_REQUIRE(K >= 1 && K <= MET_MAXK && starts && ends, "%s: K=%d ranges (1..%d)", who, K, MET_MAXK);
  r.K = K;
  for (int k = 0; k < MET_MAXK; ++k) {
    r.start[k] = r.end[k] = 0;
    c.n[k] = 0.0;
  }
  for (int k = 0; k < K; ++k) {
    const int s = starts[k], e = ends[k] == -1 ? F : ends[k];
    MRG_REQUIRE(s >= 0 && s <= e && e <= F, "%s: range %d = (%d, %d) outside [0, %d]", who, k, starts[k], ends[k],
                F);
    r.start[k] = s;
    r.end[k] = e;
    c.n[k] = rows * (double)(e - s);
  }
  return 0;
}

template <typename Elem>
static int met_run(const Elem& a, const MetRanges& r, const MetCounts& c, double* state, float* batch_out,
                   float* part, hipStream_t stream) {
  const long n = (long)a.B * a.T * a.F;
  int nb = 0;
  if (n > 0) {
    nb = met_blocks(n);
    met_partial_kernel<Elem><<<nb, 256, 0, stream>>>(a, r, part);
    if (check_launch("met_partial_kernel")) return 1;
  }
  met_final_kernel<<<1, 256, 0, stream>>>(part, nb, r.K, c, state, batch_out);
  return check_launch("met_final_kernel");
}

}  // namespace mrg

using namespace mrg;

MRG_API size_t mrg_target_metrics_workspace_bytes(int B, int T, int F) {
  // the broadcast form's per-(b, f) counts, then one row of MET_MAXK partials per block
  return ((size_t)B * F + (size_t)met_blocks((long)B * T * F) * MET_MAXK) * sizeof(float);
}

MRG_API int mrg_target_metrics_update(int B, int T, int F, const float* y, long y_bstride, const float* target,
                                      int mask_padding, int delta_start, float dscale, int K, const int* starts,
                                      const int* ends, double* state, float* batch_out, float* workspace,
                                      hipStream_t stream) {
  MRG_REQUIRE(B >= 0 && T >= 0 && F >= 1 && state && batch_out && workspace,
              "mrg_target_metrics_update: bad arguments (B=%d T=%d F=%d)", B, T, F);
  MetRanges r;
  MetCounts c;
  if (int rc = met_ranges("mrg_target_metrics_update", F, K, starts, ends, (double)B * (double)T, r, c)) return rc;
  MetPlain a;
  a.y = y; a.ys = y_bstride; a.t = target; a.B = B; a.T = T; a.F = F;
  a.mask_padding = mask_padding; a.delta_start = delta_start; a.dscale = dscale;
  return met_run(a, r, c, state, batch_out, workspace + (size_t)B * F, stream);
}

MRG_API int mrg_target_metrics_update_broadcast(int B, int T, int F, const float* y, long y_bstride,
                                                const float* target, const float* ms, long ms_bs, long ms_ts,
                                                int Tm, int t_start, float dscale, int K, const int* starts,
                                                const int* ends, double* state, float* batch_out,
                                                float* workspace, hipStream_t stream) {
  MRG_REQUIRE(B >= 0 && T >= 0 && F >= 1 && Tm >= 0 && ms && state && batch_out && workspace,
              "mrg_target_metrics_update_broadcast: bad arguments (B=%d T=%d F=%d Tm=%d)", B, T, F, Tm);
  MetRanges r;
  MetCounts c;
  if (int rc = met_ranges("mrg_target_metrics_update_broadcast", F, K, starts, ends,
                          (double)Tm * (double)B * (double)T, r, c))
    return rc;
  MetBcast a;
  a.y = y; a.ys = y_bstride; a.t = target; a.counts = workspace; a.B = B; a.T = T; a.F = F; a.Tm = Tm;
  a.t_start = t_start; a.dscale = dscale;
  if (B * F > 0) {
    met_count_kernel<<<(B * F + 255) / 256, 256, 0, stream>>>(ms, ms_bs, ms_ts, B, Tm, F, workspace);
    if (check_launch("met_count_kernel")) return 1;
  }
  return met_run(a, r, c, state, batch_out, workspace + (size_t)B * F, stream);
}
