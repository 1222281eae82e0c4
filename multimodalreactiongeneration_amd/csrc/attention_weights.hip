// Attention maps: the probabilities nn.MultiheadAttention(need_weights=True) returns, rebuilt from the
// projected Q and K and the row log-sum-exp the attention kernels saved (attention.hip keeps only O and
// lse; nothing of score size exists unless a caller asks for it here).
//
//   P[b, h, i, j] = exp(scale q_i . k_j - lse[b, h, i])   where the block-causal / padding-AND rules of
//                                                          attention.hip admit (i, j), exactly 0 elsewhere
//   extra columns (torch's order [real keys, bias key, zero key], always visible):
//                   exp(scale q_i . bias_k_h - lse), exp(-lse)        (lse: the merged one, attention_extra.hip)
//   lse is read as what it is, the row's log-sum-exp ROUNDED to one float32: that rounding (half an
//   ulp, 2.4e-7 at lse near 4) would scale a whole row, so each row is divided by the sum of its own
//   terms, taken in double (1 up to that rounding): P = exp(s - (lse + log rsum)), rows sum to 1 to
//   the last float32 rounding, and every value moves by a few 1e-7 of itself at most.
//   a row whose lse is NaN (fully hidden, no extra key) is NaN in every column, as softmax over -inf is
//   dropout: P o keep / (1 - p) with the op's key, element (b * heads + head, q, column) of rng.h's
//            attention map over the Tk + n columns (mrg_attention_keep_mask's mask): what O was built from
//
// One workgroup = 4 waves = a 64-query x 64-column tile.  The S^T sub-tiles come from qk16
// (attention_tiles.h): the MFMA chain and operand order of the forward, so s is bitwise the forward's
// and exp(s - lse) is the backward's P.  Per head the workgroup first walks every column tile some
// query of the block sees and sums the row's terms (pass 1), then forms its own tile (pass 2): the
// scores are recomputed once per column tile of the grid, Tk / 64 times in all, and no workspace or
// second launch is needed.  The bias key is one more row of the LDS key tile (row Tk) and
// the zero key a zero row, so the extra columns take the same path.  A lane's four accumulator
// registers are four consecutive columns of one query row: they go out as one 16-byte store where the
// address is 16-B aligned (row width Tk + n is often no multiple of 4, so alignment is decided per
// row), else as scalars; every row segment a wave writes is contiguous.
// average: the workgroup walks the heads in order and sums in registers (double, rounded once at the
// store; no atomics, fixed order: bitwise reproducible), then divides by the head count: out
// [B, Tq, Tk + n] instead of [B, heads, Tq, Tk + n].
// Cost: the store, 4 bytes per score at most once, and the row-sum pass, whose score products grow with
// (Tk / 64)^2 per query block.  Neither rate has been measured.
#include "mrg_common.h"
#include "rng.h"
#include "attention_tiles.h"

namespace mrg {

struct WeightArgs {
  AttnArgs a;            // q, k, lse, the padding flags, the mask rule and the dropout key
  const float* bias_k;   // [heads * D], nullable
  int W;                 // columns: Tk + extras
  float* out;
};

template <int D, bool AVG>
__global__ __launch_bounds__(256) void attn_weights_kernel(WeightArgs w) {
  using C = AttnCfg<D>;
  constexpr int C4 = D / 4;
  __shared__ __attribute__((aligned(16))) float Ks[TT * C::SA];
  const AttnArgs& a = w.a;
  // grid (column tiles, B or B * heads, query tiles)
  const int k0 = blockIdx.x * TT;
  const int b = AVG ? blockIdx.y : blockIdx.y / a.Hh;
  const int h0 = AVG ? 0 : blockIdx.y % a.Hh, h1 = AVG ? a.Hh : h0 + 1;
  const int q0 = blockIdx.z * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int qi = q0 + wave * 16 + lq;
  const bool qv = qi < a.Tq;
  const bool pad = a.qpad && a.kpad;
  const bool qp = pad && qv && a.qpad[(long)b * a.qp_bs + qi];
  const unsigned char* kpb = pad ? a.kpad + (long)b * a.Tk : nullptr;
  const int kmax = key_bound(a, qi);
  DropKey dkey = {};
  if (a.rkey) dkey = load_drop_key(a.rkey);

  const int klim = key_bound(a, q0 + 63);   // no query of the block sees a real key from here on
  // the head sum (one term without AVG) is kept in double and rounded to float once, at the store
  double acc[TT / 16][4];
#pragma unroll
  for (int sub = 0; sub < TT / 16; ++sub)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[sub][r] = 0.0;

  // the key tile at column t0 -> LDS: rows < Tk from K, row Tk the bias key, zeros beyond (the zero key
  // among them)
  auto stage_tile = [&](int t0, int hoff) {
    TileRegs<D> tk;
#pragma unroll
    for (int i = 0; i < C::NVR; ++i) {
      const int e = threadIdx.x + i * 256;
      const int row = t0 + e / C4, c = (e % C4) * 4;
      tk.r[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < TT * C4) {
        if (row < a.Tk) {
          tk.r[i] = *reinterpret_cast<const float4*>(a.k + (long)b * a.k_bs + (long)row * a.k_ts + hoff + c);
        } else if (row == a.Tk && w.bias_k) {
          const float* bp = w.bias_k + hoff + c;
          tk.r[i] = make_float4(bp[0], bp[1], bp[2], bp[3]);
        }
      }
    }
    __syncthreads();   // the reads of the tile Ks held are done
    tk.template store<C::SA>(Ks);
    __syncthreads();
  };
  // e = exp(s - lse) of column col for this lane's query, 0 where the rules hide the pair or past the row
  auto term = [&](float s, float lse, int col) -> float {
    const bool vis = col < w.W && (col >= a.Tk || (col < kmax && !(qp && kpb[col])));
    return vis ? __expf(s - lse) : 0.0f;
  };

  for (int h = h0; h < h1; ++h) {
    const int hoff = h * D;
    float qreg[C::KS];
    if (a.qvec) {
      row_values<D>(a.q + (long)b * a.q_bs + (long)min(qi, a.Tq - 1) * a.q_ts + hoff, lg, qv, qreg);
#pragma unroll
      for (int s = 0; s < C::KS; ++s) qreg[s] *= a.scale;
    } else {
#pragma unroll
      for (int s = 0; s < C::KS; ++s)
        qreg[s] = qv ? a.q[(long)b * a.q_bs + (long)qi * a.q_ts + hoff + dmap<D>(lg, s)] * a.scale : 0.0f;
    }
    const float lse = qv ? a.lse[stat_row(a, b, h, qi)] : 0.0f;
    // pass 1: rsum = sum over the row of exp(s - lse), in double.  lse is ONE float32 per row: its rounding
    // (half an ulp, 2.4e-7 at lse near 4) would scale the whole row, so the row is divided by the sum of
    // the very terms it is made of, which is 1 up to that rounding: P = exp(s - (lse + log rsum)).
    // Tiles no query of the block sees (past the causal bound, no extra column) add nothing: skipped.
    double rsum = 0.0;
    for (int t0 = 0; t0 < w.W; t0 += TT) {
      if (t0 >= klim && t0 + TT <= a.Tk) continue;   // block-uniform
      stage_tile(t0, hoff);
#pragma unroll
      for (int sub = 0; sub < TT / 16; ++sub) {
        const int kb = t0 + sub * 16;
        if (kb >= w.W) break;   // block-uniform
        const f32x4 s4 = qk16<D>(Ks, sub * 16, qreg, lq, lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) rsum += (double)term(s4[r], lse, kb + lg * 4 + r);
      }
    }
    rsum += __shfl_xor(rsum, 16, 64);   // the four lane groups of a query, in a fixed order
    rsum += __shfl_xor(rsum, 32, 64);
    const double inv = 1.0 / rsum;
    // pass 2: this block's tile
    stage_tile(k0, hoff);
#pragma unroll
    for (int sub = 0; sub < TT / 16; ++sub) {
      const int kb = k0 + sub * 16;
      if (kb >= w.W) break;   // block-uniform
      const f32x4 s4 = qk16<D>(Ks, sub * 16, qreg, lq, lg);
      Philox4 pw = {};
      if (a.rkey) pw = attn_words(dkey, (uint32_t)(b * a.Hh + h), (uint32_t)qi, (uint32_t)(kb / 4 + lg));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = term(s4[r], lse, kb + lg * 4 + r);
        double p = e == 0.0f ? 0.0 : (double)e * inv;   // hidden: exactly 0 whatever the row sum is
        if (a.rkey) p = pw.w[r] >= a.thr ? p * (double)a.keep_scale : 0.0;
        if (!(lse == lse)) p = (double)NAN;   // a fully hidden row: NaN in every column
        acc[sub][r] += p;
      }
    }
  }

  if (!qv) return;
  const double nh = (double)a.Hh;
  const long row = AVG ? (long)b * a.Tq + qi : ((long)b * a.Hh + h0) * a.Tq + qi;
  float* op = w.out + row * w.W;
#pragma unroll
  for (int sub = 0; sub < TT / 16; ++sub) {
    const int col = k0 + sub * 16 + lg * 4;
    if (col >= w.W) continue;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (float)(AVG ? acc[sub][r] / nh : acc[sub][r]);
    float* p = op + col;
    if (col + 3 < w.W && (((uintptr_t)p) & 15) == 0) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (col + r < w.W) p[r] = v[r];
    }
  }
}

}  // namespace mrg

using namespace mrg;

#define MRG_WEIGHTS_DISPATCH(AVG)                                                         \
  switch (D) {                                                                            \
    case 8: klaunch(attn_weights_kernel<8, AVG>, grid, 256, 0, stream, w); break;         \
    case 16: klaunch(attn_weights_kernel<16, AVG>, grid, 256, 0, stream, w); break;       \
    case 32: klaunch(attn_weights_kernel<32, AVG>, grid, 256, 0, stream, w); break;       \
    case 64: klaunch(attn_weights_kernel<64, AVG>, grid, 256, 0, stream, w); break;       \
  }

MRG_API int mrg_attention_weights(int B, int Hh, int Tq, int Tk, int D,
                                  const float* q, long q_bs, long q_ts, const float* k, long k_bs, long k_ts,
                                  const float* bias_k, int zero_attn, const float* lse,
                                  const unsigned char* qpad, const unsigned char* kpad, int causal, float scale,
                                  int average, unsigned int thr, float scale_keep, const unsigned long long* key,
                                  float* out, hipStream_t stream) {
  MRG_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64, "attention weights: unsupported head dim %d", D);
  MRG_REQUIRE(B >= 0 && Tq >= 0 && Tk >= 0 && Hh >= 1, "attention weights: B=%d Tq=%d Tk=%d heads=%d", B, Tq, Tk, Hh);
  MRG_REQUIRE(!causal || Tq == 0 || Tk == 0 || Tk % Tq == 0 || Tq % Tk == 0,
              "attention weights: other_modal_len must be divisible by main_modal_len (Tq=%d Tk=%d)", Tq, Tk);
  MRG_REQUIRE(Tq <= 65535 && (long)B * Hh <= 65535, "attention weights: Tq=%d and B * heads=%ld at most 65535 (grid)",
              Tq, (long)B * Hh);
  MRG_REQUIRE((long)Tk + 2 < 0x7FFFFFFFL - 64, "attention weights: Tk=%d too large", Tk);
  if (key) {
    MRG_REQUIRE((((uintptr_t)key) & 7) == 0, "attention weights: key (2 x uint64) must be 8-B aligned");
    MRG_REQUIRE(scale_keep >= 1.0f && std::isfinite(scale_keep), "attention weights: scale_keep = 1 / (1 - p), p in [0, 1)");
  }
  const int W = Tk + (bias_k ? 1 : 0) + (zero_attn ? 1 : 0);
  if (B == 0 || Tq == 0 || W == 0) return 0;
  MRG_REQUIRE(q != nullptr && lse != nullptr && out != nullptr && (k != nullptr || Tk == 0),
              "attention weights: q, k, lse and out required");
  MRG_REQUIRE(Tk == 0 || rows16(k, k_bs, k_ts), "attention weights: K rows must be 16-B aligned (strides multiple of 4 floats)");
  WeightArgs w;
  memset(&w, 0, sizeof(w));
  AttnArgs& a = w.a;
  a.q = q; a.q_bs = q_bs; a.q_ts = q_ts; a.k = k; a.k_bs = k_bs; a.k_ts = k_ts;
  a.lse = const_cast<float*>(lse); a.qpad = qpad; a.kpad = kpad;
  a.B = B; a.Hh = Hh; a.Tq = Tq; a.Tk = Tk; a.causal = (causal && Tk > 0) ? 1 : 0; a.scale = scale;
  a.q_off = 0; a.Tqf = Tq; a.qp_bs = Tq; a.st_ld = Tq; a.st_off = 0;
  a.qvec = rows16(q, q_bs, q_ts);
  a.rkey = key; a.thr = thr; a.keep_scale = scale_keep;
  w.bias_k = bias_k; w.W = W; w.out = out;
  const dim3 grid((unsigned)((W + TT - 1) / TT), (unsigned)(average ? B : B * Hh), (unsigned)((Tq + 63) / 64));
  if (average) {
    MRG_WEIGHTS_DISPATCH(true);
  } else {
    MRG_WEIGHTS_DISPATCH(false);
  }
  return check_launch("attn_weights_kernel");
}
