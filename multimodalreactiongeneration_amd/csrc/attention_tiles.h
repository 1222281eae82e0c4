// The attention kernels' argument block, mask rule and S^T tile toolkit, shared by attention.hip (the
// forward and the backward passes) and attention_weights.hip (the probabilities rebuilt from the
// saved log-sum-exp): one definition of how a score tile is formed, so every kernel that recomputes
// S = scale Q K^T gets the bits the forward got.
#pragma once
#include "mrg_common.h"

namespace mrg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AttnArgs {
  const float* q; long q_bs, q_ts;
  const float* k; long k_bs, k_ts;
  const float* v; long v_bs, v_ts;
  float* o; long o_bs, o_ts;
  float* lse;  // [B, Hh, Tq]
  const unsigned char* qpad;  // [B, Tq] nullable
  const unsigned char* kpad;  // [B, Tk] nullable
  const float* dout; long do_bs, do_ts;
  float* dlt;  // [B, Hh, Tq]
  float* dq; long dq_bs, dq_ts;
  float* dk; long dk_bs, dk_ts;
  float* dv; long dv_bs, dv_ts;
  int B, Hh, Tq, Tk;
  int causal;
  float scale;
  int qvec, ovec, dkvvec;  // rows of q / o / dk and dv 16-B aligned: float4 loads and stores
  // query chunk (mrg_attention_*_chunk): the Tq queries are rows [q_off, q_off + Tq) of a sequence of
  // Tqf queries (the causal rule uses global indices and Tk / Tqf); qpad rows have stride qp_bs;
  // kv_acc: the dK / dV pass adds into dk / dv (a chunk's share) instead of storing
  int q_off, Tqf;
  long qp_bs;
  int kv_acc;
  // lse / delta rows: [B, Hh, st_ld] arrays, this call's queries at column st_off (chunk calls hand in
  // the whole sequence's statistics: st_ld = Tqf, st_off = q_off)
  int st_ld, st_off;
  // attention-probability dropout (the DROP instantiations only; rng.h): the op's 16-byte key in
  // device memory, the keep threshold and 1 / (1 - p)
  const unsigned long long* rkey;
  uint32_t thr;
  float keep_scale;
};

// host: the rows of a [B, T, ...] operand (pointer, batch and row stride in floats) are 16-B aligned, so
// float4 loads and stores apply; an operand that is not there passes
inline bool rows16(const void* p, long bs, long ts) {
  return p == nullptr || ((((uintptr_t)p) & 15) == 0 && (bs & 3) == 0 && (ts & 3) == 0);
}

__device__ __forceinline__ long stat_row(const AttnArgs& a, int b, int h, int qi) {
  return ((long)b * a.Hh + h) * a.st_ld + a.st_off + qi;
}

// exclusive upper bound of the keys query i may see (causal rule only; Tk when not causal)
__device__ __forceinline__ int key_bound(const AttnArgs& a, int i) {
  if (!a.causal) return a.Tk;
  i = min(i, a.Tq - 1) + a.q_off;
  int lim = (a.Tk >= a.Tqf) ? (i + 1) * (a.Tk / a.Tqf) : i / (a.Tqf / a.Tk) + 1;
  return min(lim, a.Tk);
}

static constexpr int TT = 64;  // keys (forward, dQ) or queries (dK/dV) per LDS tile

template <int D>
struct AttnCfg {
  static constexpr int DT = (D + 15) / 16;  // 16-wide d tiles of the output
  static constexpr int DP = DT * 16;
  static constexpr int KS = D / 4;          // k-steps over d
  // VEC (D >= 32): lane group lg takes the contiguous contraction indices d = KS*lg + s and the
  // output columns d = DT*i + dt, so LDS operands are read as float4 / float2 (4x fewer LDS
  // instructions than one ds_read_b32 per MFMA) and outputs are stored as contiguous runs; the
  // sums are the same, in a different order.  D < 32 keeps the interleaved map (d = 4s + lg).
  static constexpr bool VEC = D >= 32;
  static constexpr int SA = VEC ? DP + 4 : DP + 2;  // row stride for the [row = lane&15][d] operand reads
  static constexpr int SV = DP + 4;         // row stride for [row = 4(lane>>4)+s][16dt + lane&15] reads
  static constexpr int NV = TT * (D / 4) / 256;  // float4 per thread per tile (0 at D = 8: half the threads load)
  static constexpr int NVR = NV > 0 ? NV : 1;
};

// TT rows x D of a [T, ...] operand -> registers (float4, zero past nrows), then -> LDS.
template <int D>
struct TileRegs {
  float4 r[AttnCfg<D>::NVR];
  __device__ __forceinline__ void load(const float* base, long ts, int r0, int nrows) {
    constexpr int C4 = D / 4;
#pragma unroll
    for (int i = 0; i < AttnCfg<D>::NVR; ++i) {
      const int e = threadIdx.x + i * 256;
      const int row = e / C4, c = (e % C4) * 4;
      r[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < TT * C4 && r0 + row < nrows) r[i] = *reinterpret_cast<const float4*>(base + (long)(r0 + row) * ts + c);
    }
  }
  template <int S>
  __device__ __forceinline__ void store(float* lds) const {
    constexpr int C4 = D / 4;
#pragma unroll
    for (int i = 0; i < AttnCfg<D>::NVR; ++i) {
      const int e = threadIdx.x + i * 256;
      if (e < TT * C4) {
        const int row = e / C4, c = (e % C4) * 4;
        float* p = lds + row * S + c;
        if (S % 4 == 0) {
          *reinterpret_cast<float4*>(p) = r[i];
        } else {
          *reinterpret_cast<float2*>(p) = make_float2(r[i].x, r[i].y);
          *reinterpret_cast<float2*>(p + 2) = make_float2(r[i].z, r[i].w);
        }
      }
    }
  }
};

// contraction index d of k-step s for lane group lg (same map for every operand of a product)
template <int D>
__device__ __forceinline__ int dmap(int lg, int s) {
  return AttnCfg<D>::VEC ? AttnCfg<D>::KS * lg + s : 4 * s + lg;
}
// the KS contraction operands of LDS row `row` for this lane: v[s] = S[row * STR + dmap(lg, s)]
template <int D, int STR>
__device__ __forceinline__ void row_operands(const float* S, int row, int lg, float (&v)[AttnCfg<D>::KS]) {
  using C = AttnCfg<D>;
  if constexpr (C::VEC) {
#pragma unroll
    for (int i = 0; i < C::KS; i += 4) {
      const float4 t = *reinterpret_cast<const float4*>(S + row * STR + C::KS * lg + i);
      v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < C::KS; ++s) v[s] = S[row * STR + 4 * s + lg];
  }
}

// this lane's KS contraction values of one row (row pointer p, 16-B aligned): v[s] = p[dmap(lg, s)]
// (float4 loads when the map is lane-contiguous), zero when !valid
template <int D>
__device__ __forceinline__ void row_values(const float* p, int lg, bool valid, float (&v)[AttnCfg<D>::KS]) {
  using C = AttnCfg<D>;
  if constexpr (C::VEC) {
#pragma unroll
    for (int i = 0; i < C::KS; i += 4) {
      const float4 t = valid ? *reinterpret_cast<const float4*>(p + C::KS * lg + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < C::KS; ++s) v[s] = valid ? p[4 * s + lg] : 0.0f;
  }
}

// S^T tile (16 keys x 16 queries) = K rows [kr..kr+15] . Q^T, two accumulation chains
template <int D>
__device__ __forceinline__ f32x4 qk16(const float* Ks, int rowbase, const float (&qreg)[AttnCfg<D>::KS], int lq,
                                      int lg) {
  using C = AttnCfg<D>;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
  float kv[C::KS];
  row_operands<D, C::SA>(Ks, rowbase + lq, lg, kv);
#pragma unroll
  for (int s = 0; s < C::KS; s += 2) {
    s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[s], qreg[s], s0, 0, 0, 0);
    if (s + 1 < C::KS) s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[s + 1], qreg[s + 1], s1, 0, 0, 0);
  }
  return s0 + s1;
}

}  // namespace mrg
