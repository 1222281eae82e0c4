// The always-visible extra keys of nn.MultiheadAttention(add_bias_kv / add_zero_attn), merged into the
// result of the attention kernels (attention.hip) instead of being appended to K and V.
//
// torch appends bias_k / bias_v as one more key / value row per sample and, after the head split, one
// more all-zero key / value per (sample, head); no mask rule hides them.  They are the same for every
// query of a (sample, head), so the softmax over [K; extras] is the log-sum-exp merge of the main
// kernel's row with at most two scalar scores per (b, head, q):
//   s1 = scale q_h . bias_k_h (the bias key), s0 = 0 (the zero key)
//   lse_tot = logaddexp(lse_main, s1, s0), w_main = exp(lse_main - lse_tot), w1 = exp(s1 - lse_tot)
//   O = w_main O_main + w1 m1 bias_v_h            (m1 = keep / (1 - p) of attention element k = Tk)
// The main backward, handed the merged O and lse_tot, recomputes P = exp(s - lse_tot) and so gives the
// main keys' share of dQ, dK and dV; the extras' share is
//   dS1 = w1 (m1 dO_h . bias_v_h - delta), delta = rowsum(dO_h o O_h)
//   dq_h += scale dS1 bias_k_h, dbias_k_h = scale sum_(b,q) dS1 q_h, dbias_v_h = sum_(b,q) w1 m1 dO_h
// (the zero key has a zero key and a zero value: no gradient).
// The dropout backward of attention.hip forms delta from the main keys' own terms, rowsum(P o dP), so
// there it lacks the bias key's term c = w1 m1 dO_h . bias_v_h.  The correction is linear in c:
//   dq_h -= scale c sum_k P_k K_k     (sum_k P_k K_k = w_main softmax_main(S) K: a forward call with V = K)
//   dK_k -= scale sum_q c_q P_qk q_q  (the dK / dV pass with dO = 0 and c in the delta rows)
// so mrg_attention_extra_bwd takes that forward's result (pk, lse_main), applies the dq term and
// writes c for the second.
//
// Kernels: row-parallel and HBM-bound.  One wave owns one (b, q) row of E = heads * D floats; a lane
// owns one unit (a float4 where every row is 16-B aligned, else one float) per 64-unit step, a head is
// G = D / unit-width neighbouring lanes (G divides 64), and the per-head dot products are xor shuffles
// inside the group.  Every element of o / dq is read and written by the one lane that owns it, so the
// in-place update needs no ordering.  dbias_k / dbias_v: lane registers over the wave's rows, the
// block's four waves summed through LDS in wave order, one partial row per block, and a second kernel
// that adds the blocks' partials in block order: no atomics, the same bits on every run.
#include "mrg_common.h"
#include "rng.h"
#include "attention_tiles.h"   // rows16

namespace mrg {

static constexpr int XE_MAX = 1024;   // widest row (the residual LayerNorm's bound as well)
static constexpr int XB_MAX = 256;    // most blocks of the backward (= partial rows of the reducer)

struct ExtraArgs {
  const float* q; long q_bs, q_ts;
  const float* bias_k;   // [E], nullable together with bias_v
  const float* bias_v;
  float* o; long o_bs, o_ts;
  float* lse;            // [B, Hh, Tq]: lse_main in, lse_tot out (forward); lse_tot (backward)
  const float* dout; long do_bs, do_ts;
  float* dq; long dq_bs, dq_ts;
  const float* pk; long pk_bs, pk_ts;   // softmax_main(S) K (dropout backward), nullable
  const float* lse_main;                // [B, Hh, Tq] of that call
  float* cbuf;                          // [B, Hh, Tq] out: c
  float* part;                          // [blocks][2][E] partial dbias_k / dbias_v
  int B, Hh, Tq, Tk, D, E;
  int zero;
  float scale;
  const unsigned long long* rkey;       // nullable: no dropout
  uint32_t thr;
  float keep_scale;
};

template <int W>
struct Unit {
  float v[W];
};

template <int W>
__device__ __forceinline__ Unit<W> ld_unit(const float* p) {
  Unit<W> u;
  if constexpr (W == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    u.v[0] = t.x; u.v[1] = t.y; u.v[2] = t.z; u.v[3] = t.w;
  } else {
    u.v[0] = *p;
  }
  return u;
}

template <int W>
__device__ __forceinline__ void st_unit(float* p, const Unit<W>& u) {
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(u.v[0], u.v[1], u.v[2], u.v[3]);
  } else {
    *p = u.v[0];
  }
}

template <int W>
__device__ __forceinline__ float dot_unit(const Unit<W>& a, const Unit<W>& b) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < W; ++i) s = fmaf(a.v[i], b.v[i], s);
  return s;
}

// sum over the G neighbouring lanes of a head (G a power of two, wave-uniform)
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int off = G >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// keep / (1 - p) of attention element (b, head, q, k = Tk): the bias key's column
__device__ __forceinline__ float bias_keep(const ExtraArgs& a, const DropKey& dk, int b, int head, int qi) {
  if (!a.rkey) return 1.0f;
  const Philox4 w = attn_words(dk, (uint32_t)(b * a.Hh + head), (uint32_t)qi, (uint32_t)(a.Tk >> 2));
  const int i = a.Tk & 3;
  const uint32_t word = i == 0 ? w.w[0] : i == 1 ? w.w[1] : i == 2 ? w.w[2] : w.w[3];
  return word >= a.thr ? a.keep_scale : 0.0f;
}

// a row the main kernel found fully masked (lse NaN there; -inf is taken as well)
__device__ __forceinline__ bool row_dead(float lse) { return !(lse == lse) || lse == -INFINITY; }

template <int W>
__global__ __launch_bounds__(256) void attn_extra_fwd_kernel(ExtraArgs a) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)a.B * a.Tq) return;   // wave-uniform
  const int b = (int)(row / a.Tq), qi = (int)(row % a.Tq);
  const int units = a.E / W, G = a.D / W;
  const bool has_b = a.bias_k != nullptr;
  DropKey dk = {};
  if (a.rkey) dk = load_drop_key(a.rkey);
  const float* qr = a.q + (long)b * a.q_bs + (long)qi * a.q_ts;
  float* orow = a.o + (long)b * a.o_bs + (long)qi * a.o_ts;
  for (int u0 = 0; u0 < units; u0 += 64) {
    const int u = u0 + lane;
    const bool act = u < units;       // whole head groups: G divides 64 and units
    const int e = u * W, head = act ? u / G : 0;
    float s1 = 0.0f;
    Unit<W> bv = {};
    if (has_b) {
      float d = 0.0f;
      if (act) {
        d = dot_unit<W>(ld_unit<W>(qr + e), ld_unit<W>(a.bias_k + e));
        bv = ld_unit<W>(a.bias_v + e);
      }
      s1 = group_sum(d, G) * a.scale;
    }
    if (!act) continue;
    const long si = ((long)b * a.Hh + head) * a.Tq + qi;
    const float lm = a.lse[si];
    const bool dead = row_dead(lm);
    float m = dead ? -INFINITY : lm;
    if (has_b) m = fmaxf(m, s1);
    if (a.zero) m = fmaxf(m, 0.0f);
    float sum = dead ? 0.0f : __expf(lm - m);
    if (has_b) sum += __expf(s1 - m);
    if (a.zero) sum += __expf(-m);
    const float lt = m + __logf(sum);
    const float wm = dead ? 0.0f : __expf(lm - lt);
    const float w1 = has_b ? __expf(s1 - lt) * bias_keep(a, dk, b, head, qi) : 0.0f;
    Unit<W> ov = ld_unit<W>(orow + e);
#pragma unroll
    for (int i = 0; i < W; ++i) ov.v[i] = (dead ? 0.0f : wm * ov.v[i]) + w1 * bv.v[i];   // never 0 * NaN
    st_unit<W>(orow + e, ov);
    if ((lane & (G - 1)) == 0) a.lse[si] = lt;
  }
}

// MAXI: most 64-unit steps of a row (E <= XE_MAX): the lane's dbias accumulators are registers
template <int W>
__global__ __launch_bounds__(256) void attn_extra_bwd_kernel(ExtraArgs a) {
  constexpr int MAXI = XE_MAX / (64 * W);
  extern __shared__ __attribute__((aligned(16))) float xlds[];   // [4 waves][2][E]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int units = a.E / W, G = a.D / W;
  const long rows = (long)a.B * a.Tq;
  DropKey dk = {};
  if (a.rkey) dk = load_drop_key(a.rkey);
  Unit<W> gk[MAXI], gv[MAXI];
#pragma unroll
  for (int it = 0; it < MAXI; ++it)
#pragma unroll
    for (int i = 0; i < W; ++i) gk[it].v[i] = gv[it].v[i] = 0.0f;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const int b = (int)(row / a.Tq), qi = (int)(row % a.Tq);
    const float* qr = a.q + (long)b * a.q_bs + (long)qi * a.q_ts;
    const float* orow = a.o + (long)b * a.o_bs + (long)qi * a.o_ts;
    const float* dor = a.dout + (long)b * a.do_bs + (long)qi * a.do_ts;
    float* dqr = a.dq + (long)b * a.dq_bs + (long)qi * a.dq_ts;
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
      if (it * 64 >= units) break;     // wave-uniform
      const int u = it * 64 + lane;
      const bool act = u < units;
      const int e = u * W, head = act ? u / G : 0;
      Unit<W> qv = {}, kv = {}, vv = {}, dv = {};
      float dqk = 0.0f, dbv = 0.0f, dlt = 0.0f;
      if (act) {
        qv = ld_unit<W>(qr + e);
        kv = ld_unit<W>(a.bias_k + e);
        vv = ld_unit<W>(a.bias_v + e);
        dv = ld_unit<W>(dor + e);
        dqk = dot_unit<W>(qv, kv);
        dbv = dot_unit<W>(dv, vv);
        dlt = dot_unit<W>(dv, ld_unit<W>(orow + e));
      }
      dqk = group_sum(dqk, G);
      dbv = group_sum(dbv, G);
      dlt = group_sum(dlt, G);
      if (!act) continue;
      const long si = ((long)b * a.Hh + head) * a.Tq + qi;
      const float lt = a.lse[si];
      const float w1m = __expf(dqk * a.scale - lt) * bias_keep(a, dk, b, head, qi);   // w1 m1
      const float c = w1m * dbv;
      const float ds = (c - __expf(dqk * a.scale - lt) * dlt) * a.scale;               // scale dS1
      Unit<W> dqv = ld_unit<W>(dqr + e);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        dqv.v[i] = fmaf(ds, kv.v[i], dqv.v[i]);
        gk[it].v[i] = fmaf(ds, qv.v[i], gk[it].v[i]);
        gv[it].v[i] = fmaf(w1m, dv.v[i], gv[it].v[i]);
      }
      if (a.pk) {   // the dropout backward's missing delta term
        const float l2 = a.lse_main[si];
        const float f = row_dead(l2) ? 0.0f : -a.scale * c * __expf(l2 - lt);
        if (f != 0.0f) {
          const Unit<W> pv = ld_unit<W>(a.pk + (long)b * a.pk_bs + (long)qi * a.pk_ts + e);
#pragma unroll
          for (int i = 0; i < W; ++i) dqv.v[i] = fmaf(f, pv.v[i], dqv.v[i]);
        }
        if ((lane & (G - 1)) == 0) a.cbuf[si] = c;
      }
      st_unit<W>(dqr + e, dqv);
    }
  }
  // the block's partial: waves 0..3 in order
  float* mine = xlds + (long)wave * 2 * a.E;
#pragma unroll
  for (int it = 0; it < MAXI; ++it) {
    const int u = it * 64 + lane;
    if (u < units) {
      st_unit<W>(mine + u * W, gk[it]);
      st_unit<W>(mine + a.E + u * W, gv[it]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * a.E; i += 256) {
    float s = xlds[i];
#pragma unroll
    for (int w = 1; w < 4; ++w) s += xlds[(long)w * 2 * a.E + i];
    a.part[(long)blockIdx.x * 2 * a.E + i] = s;
  }
}

// dbias_k | dbias_v [E] each: the blocks' partial rows added in block order
__global__ __launch_bounds__(256) void attn_extra_reduce_kernel(const float* part, int nblk, int E, float* dbk,
                                                                float* dbv, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * E) return;
  float s = 0.0f;
  for (int j = 0; j < nblk; ++j) s += part[(long)j * 2 * E + i];
  float* out = i < E ? dbk + i : dbv + (i - E);
  *out = accumulate ? *out + s : s;
}

}  // namespace mrg

using namespace mrg;

static int extra_check(int B, int Hh, int Tq, int Tk, int D, float keep_scale, const unsigned long long* rkey) {
  MRG_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64, "attention extra keys: unsupported head dim %d", D);
  MRG_REQUIRE(B >= 0 && Tq >= 0 && Tk >= 0 && Hh >= 1 && (long)Hh * D <= XE_MAX,
              "attention extra keys: B=%d Tq=%d Tk=%d heads=%d (heads * D at most %d)", B, Tq, Tk, Hh, XE_MAX);
  MRG_REQUIRE((long)B * Hh < 0xFFFFFFFFL && (long)B * Tq < 0x7FFFFFFFL * 4, "attention extra keys: B * heads / B * Tq too large");
  if (rkey) {
    MRG_REQUIRE((((uintptr_t)rkey) & 7) == 0, "attention extra keys: key (2 x uint64) must be 8-B aligned");
    MRG_REQUIRE(keep_scale >= 1.0f && std::isfinite(keep_scale), "attention extra keys: scale_keep = 1 / (1 - p), p in [0, 1)");
  }
  return 0;
}

static int extra_blocks(long rows) {
  const long nb = (rows + 3) / 4;
  return (int)(nb < XB_MAX ? nb : XB_MAX);
}

MRG_API int mrg_attention_extra_fwd(int B, int Hh, int Tq, int D, const float* q, long q_bs, long q_ts,
                                    const float* bias_k, const float* bias_v, int zero_attn, float scale,
                                    float* o, long o_bs, long o_ts, float* lse, int Tk, unsigned int thr,
                                    float keep_scale, const unsigned long long* rkey, hipStream_t stream) {
  if (int e = extra_check(B, Hh, Tq, Tk, D, keep_scale, rkey)) return e;
  MRG_REQUIRE((bias_k == nullptr) == (bias_v == nullptr), "attention extra keys: bias_k and bias_v come together");
  MRG_REQUIRE(bias_k != nullptr || zero_attn, "attention extra keys: neither a bias key nor a zero key requested");
  MRG_REQUIRE(o != nullptr && lse != nullptr && (q != nullptr || bias_k == nullptr),
              "attention extra keys fwd: q, o and lse required");
  if (B == 0 || Tq == 0) return 0;
  ExtraArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.q_bs = q_bs; a.q_ts = q_ts; a.bias_k = bias_k; a.bias_v = bias_v;
  a.o = o; a.o_bs = o_bs; a.o_ts = o_ts; a.lse = lse;
  a.B = B; a.Hh = Hh; a.Tq = Tq; a.Tk = Tk; a.D = D; a.E = Hh * D; a.zero = zero_attn ? 1 : 0; a.scale = scale;
  a.rkey = bias_k ? rkey : nullptr; a.thr = thr; a.keep_scale = keep_scale;   // the zero key's value is 0: kept or not
  const bool vec = rows16(q, q_bs, q_ts) && rows16(o, o_bs, o_ts) && rows16(bias_k, 0, 0) && rows16(bias_v, 0, 0);
  const dim3 grid((unsigned)(((long)B * Tq + 3) / 4));
  if (vec) klaunch(attn_extra_fwd_kernel<4>, grid, 256, 0, stream, a);
  else klaunch(attn_extra_fwd_kernel<1>, grid, 256, 0, stream, a);
  return check_launch("attn_extra_fwd_kernel");
}

MRG_API size_t mrg_attention_extra_bwd_workspace_bytes(int B, int Hh, int Tq, int D) {
  if (B <= 0 || Tq <= 0 || Hh <= 0 || D <= 0) return 0;
  return (size_t)extra_blocks((long)B * Tq) * 2 * Hh * D * sizeof(float);
}

MRG_API int mrg_attention_extra_bwd(int B, int Hh, int Tq, int D, const float* q, long q_bs, long q_ts,
                                    const float* bias_k, const float* bias_v, float scale,
                                    const float* o, long o_bs, long o_ts, const float* lse,
                                    const float* dout, long do_bs, long do_ts, float* dq, long dq_bs, long dq_ts,
                                    float* dbias_k, float* dbias_v, int accumulate, int Tk, unsigned int thr,
                                    float keep_scale, const unsigned long long* rkey,
                                    const float* pk, long pk_bs, long pk_ts, const float* lse_main, float* cbuf,
                                    float* workspace, hipStream_t stream) {
  if (int e = extra_check(B, Hh, Tq, Tk, D, keep_scale, rkey)) return e;
  MRG_REQUIRE(bias_k != nullptr && bias_v != nullptr,
              "attention extra keys bwd: bias_k and bias_v required (the zero key has no gradient: no call)");
  MRG_REQUIRE(q != nullptr && o != nullptr && lse != nullptr && dout != nullptr && dq != nullptr &&
              dbias_k != nullptr && dbias_v != nullptr, "attention extra keys bwd: null buffer");
  MRG_REQUIRE((pk == nullptr) == (lse_main == nullptr) && (pk == nullptr) == (cbuf == nullptr),
              "attention extra keys bwd: pk, lse_main and cbuf come together");
  MRG_REQUIRE(pk == nullptr || rkey != nullptr, "attention extra keys bwd: the delta correction belongs to the dropout backward");
  const int E = Hh * D;
  if (B == 0 || Tq == 0) {
    if (!accumulate) {
      MRG_HIP(hipMemsetAsync(dbias_k, 0, (size_t)E * sizeof(float), stream));
      MRG_HIP(hipMemsetAsync(dbias_v, 0, (size_t)E * sizeof(float), stream));
    }
    return 0;
  }
  MRG_REQUIRE(workspace != nullptr, "attention extra keys bwd: workspace (mrg_attention_extra_bwd_workspace_bytes) required");
  ExtraArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.q_bs = q_bs; a.q_ts = q_ts; a.bias_k = bias_k; a.bias_v = bias_v;
  a.o = const_cast<float*>(o); a.o_bs = o_bs; a.o_ts = o_ts; a.lse = const_cast<float*>(lse);
  a.dout = dout; a.do_bs = do_bs; a.do_ts = do_ts; a.dq = dq; a.dq_bs = dq_bs; a.dq_ts = dq_ts;
  a.pk = pk; a.pk_bs = pk_bs; a.pk_ts = pk_ts; a.lse_main = lse_main; a.cbuf = cbuf; a.part = workspace;
  a.B = B; a.Hh = Hh; a.Tq = Tq; a.Tk = Tk; a.D = D; a.E = E; a.scale = scale;
  a.rkey = rkey; a.thr = thr; a.keep_scale = keep_scale;
  const bool vec = rows16(q, q_bs, q_ts) && rows16(o, o_bs, o_ts) && rows16(dout, do_bs, do_ts) && rows16(dq, dq_bs, dq_ts) &&
                   rows16(pk, pk_bs, pk_ts) && rows16(bias_k, 0, 0) && rows16(bias_v, 0, 0);
  const int nblk = extra_blocks((long)B * Tq);
  const unsigned lds = 4u * 2u * (unsigned)E * sizeof(float);   // at most 32 KB
  if (vec) klaunch(attn_extra_bwd_kernel<4>, dim3(nblk), 256, lds, stream, a);
  else klaunch(attn_extra_bwd_kernel<1>, dim3(nblk), 256, lds, stream, a);
  if (check_launch("attn_extra_bwd_kernel")) return 1;
  klaunch(attn_extra_reduce_kernel, dim3((2 * E + 255) / 256), 256, 0, stream, (const float*)workspace, nblk, E,
          dbias_k, dbias_v, accumulate ? 1 : 0);
  return check_launch("attn_extra_reduce_kernel");
}
