// Fused per-frame kernels of lstmformer generation (Metaformer.prediction -> head_motion_generation
// -> generate_one_step, mr_gen/model/lstmformer/lstmformer.py:426-521).
//
// Every generated frame is a T = 1 forward with zero recurrent state and empty lead
// inputs (gen_dummy_input, :549-559).  What depends on the previous frame is only the MAIN chain
// (self motion -> feature_embedding.0 -> per block: LSTM mixer, two integrators, cat_linear,
// FeedForward -> output FeedForward -> y -> next frame's self motion).  The other modalities' block-0
// encoders and, at one audio frame per prediction frame, the integrators' whole attention output
// (one visible key: softmax weight exactly 1, so MHA(q, kv) = out_proj(V(kv)) whatever q is) are
// computed for all frames at once by the host (generate.py) as large GEMMs.  Per frame and block
// this file then runs five launches instead of ~30:
//
//   gen_lstm    X = LN(ffn(prev) + prev) (block 0: X = ms_in W_fe^T + b_fe), gates = X W_ih^T + b,
//               zero-state cell -> h                                    (mixer_block.py:237-252)
//               (a GRU mixer: gen_gru, gates = X W_ih^T + b_ih, zero-state GRU cell, mixer_block.py:193-208)
//   gen_linear  Y = LN(h + X), Z = Y W^T + b                           (mixer_block.py:479-507)
//   gen_linear  M = LN(Z + Y), Y_i = LN(a_i + M), Z_i = Y_i W_i^T + b_i  (both integrators,
//               mixer_block.py:567-603)
//   gen_linear  C = [LN(Z_0 + Y_0) | LN(Z_1 + Y_1)], M3 = C W_cat^T + b  (multi_modal_metaformer.py:128-217)
//   gen_ffn     Zf = relu(M3 W1^T + b1) W2^T + b2                       (multi_modal_metaformer.py:328)
//
// and one gen_ffn for the output FeedForward with the sampling select of :487-492 folded in
// (ms_in(t + 1) = mask[t] ? y(t) : motion_s[t]).  Each launch owns 16 batch rows x 16 output
// columns per workgroup; the LayerNorms a stage consumes are recomputed from their inputs in the
// workgroup's prologue (16 rows x 256, L2-resident) instead of a launch of their own, and each
// workgroup writes its share of the normalised rows the next stage needs as a residual.
//
// At r > 1 audio frames per prediction frame (1 < r <= 16) the audio integrator's query sees r keys,
// so its attention output depends on the query and stays in the frame loop; its keys and values
// (the audio encoder's output through W_k / W_v) are still hoisted.  Three launches then sit between
// the second and the third above, eight per block:
//
//   gen_linear     Q = LN(Z + Y) W_q^T + b_q                            (mode 0 again, rows not kept)
//   gen_attention  ctx = softmax(Q_h K_h^T / sqrt(D)) V_h per head over the frame's r keys
//   (few-row GEMM) a_0 = ctx W_o^T + b_o, the a_0 of the two-integrator launch
//
// Products on v_mfma_f32_16x16x4_f32 (exact fp32 multiply-adds; the k order differs from the
// training kernels', fp32 class).  E = 256, FeedForward bottleneck 64 (the lstmformer config).
#include "gen_loop.h"

namespace mrg {

static constexpr int GR = 16;    // batch rows per workgroup

struct GenLstmArgs {
  int B, fm;
  const float* ms;               // PRO 0: self-motion input [B][fm]
  const float* fe_w;             // feature_embedding.0 [GE][fm], bias [GE]
  const float* fe_b;
  const float* a;                // PRO 1: X = LN(a + r) (the previous block's FeedForward)
  const float* r;
  const float* ga;
  const float* be;
  float eps;
  float* xw;                     // X [B][GE] (this block's residual input), each workgroup its share
  const float* w_ih;             // [4 GE][GE] (gen_gru_kernel: [3 GE][GE], gates r, z, n)
  const float* b_ih;
  const float* b_hh;
  float* h;                      // [B][GE]
};

struct GenLinArgs {
  int B;
  const float* a[2];             // first LayerNorm inputs (PRO 2: the two halves)
  const float* r[2];
  const float* ga[2];
  const float* be[2];
  long lda;                      // row stride of a / r / a2
  const float* a2[2];            // PRO 1: second LayerNorm: Y_i = LN(a2[i] + LN(a + r))
  const float* ga2[2];
  const float* be2[2];
  float eps;
  float* xw;                     // the normalised input rows (nullable), each workgroup its share
  long ldxw;
  const float* w[2];             // weight [n][K] of the column half (PRO 1: per integrator)
  const float* bias[2];
  float* out;
  long ldo;
};

struct GenFfnArgs {
  int B, N;                      // N output columns (256, or fm for the output FeedForward)
  const float* a;                // PRO 0: X = a; PRO 1: X = LN(a + r)
  const float* r;
  const float* ga;
  const float* be;
  float eps;
  const float* w1;               // [GHB][GE]
  const float* b1;
  const float* w2;               // [N][GHB]
  const float* b2;
  float* out;                    // OUT 0: [B][N]
  float* pred;                   // OUT 1: pred[b * pred_bs + t * N + n]
  long pred_bs;
  float* ms_next;                // OUT 1: [B][N] = mask[t] ? y : ms_src
  const float* ms_src;           // motion_s frame t [B][N]
  const unsigned char* mask;     // [T] on the device
  int t;
};


// Every launch below first issues the loads that do not depend on the previous launch (this lane's
// weight fragments, gl_wload; the LayerNorm gamma / beta; the biases of its outputs), then all of its
// activation rows (gen_rows_ld: clamped past B; zeroed after, gen_row_put) before the first LayerNorm
// reduction, so a kernel waits about one memory round trip before its products (gl_mma, gen_loop.h).

// Rows wave + 4 i (i < 4) of this workgroup's 16 of N [B][ld] inputs, the lane's four columns, into
// x[input][i]; rows past B read row B - 1 (in bounds, no branch around a load)
template <int N>
__device__ __forceinline__ void gen_rows_ld(const float* const* src, long ld, int row0, int B, int wave, int lane,
                                            float4 (*x)[GR / 4]) {
#pragma unroll
  for (int i = 0; i < GR / 4; ++i) {
    const long at = (long)min(row0 + wave + 4 * i, B - 1) * ld + 4 * lane;
#pragma unroll
    for (int j = 0; j < N; ++j) x[j][i] = gen_ld4(src[j] + at);
  }
}
// Is column k in this workgroup's share of the 256-wide rows that `tiles` column tiles write back between them?
__device__ __forceinline__ bool gen_my_share(int k, int tiles) {
  const int share = GE / tiles, sh0 = (blockIdx.x % tiles) * share;
  return k >= sh0 && k < sh0 + share;
}
// Four columns of batch row b: zero past B, else to xw[at] when they are this workgroup's to keep (xw
// null: not kept); to LDS
__device__ __forceinline__ void gen_row_put(float4 v, int b, int B, float* xw, long at, float* xs) {
  if (xw && b < B) *reinterpret_cast<float4*>(xw + at) = v;
  if (b >= B) v = gen_zero4();
  *reinterpret_cast<float4*>(xs) = v;
}

// The recurrent mixers' input rows X [16][GE] of this workgroup into xs (rows past B zero), and its
// share (GE / gridDim.x columns) of them into p.xw.  PRO 0: X = ms W_fe^T + b_fe; PRO 1: X = LN(a + r)
template <int PRO>
__device__ __forceinline__ void gen_mixer_x(const GenLstmArgs& p, float (*xs)[GE + 4], float (*msl)[16]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * GR;
  if (PRO == 0) {
    // X = ms W_fe^T + b_fe (K = fm <= 16): the 16 rows' inputs staged in LDS, thread = column
    const int k = tid;
    float wf[16];
#pragma unroll
    for (int f = 0; f < 16; ++f) wf[f] = f < p.fm ? p.fe_w[k * p.fm + f] : 0.0f;
    const float bk = p.fe_b[k];
    if (tid < GR * 16) {
      const int m = tid >> 4, f = tid & 15;
      msl[m][f] = (f < p.fm && row0 + m < p.B) ? p.ms[(long)(row0 + m) * p.fm + f] : 0.0f;
    }
    __syncthreads();
    const bool mine = gen_my_share(k, gridDim.x);
#pragma unroll
    for (int m = 0; m < GR; ++m) {
      float s = 0.0f;
#pragma unroll
      for (int f = 0; f < 16; ++f) s = fmaf(msl[m][f], wf[f], s);
      const float v = row0 + m < p.B ? s + bk : 0.0f;
      if (mine && row0 + m < p.B) p.xw[(long)(row0 + m) * GE + k] = v;
      xs[m][k] = v;
    }
  } else {
    const GlLn ln = gl_lnp(p.ga, p.be, lane);
    const float* src[2] = {p.a, p.r};
    float4 x[2][GR / 4];
    gen_rows_ld<2>(src, GE, row0, p.B, wave, lane, x);
    const int k = 4 * lane;
    float* keep = gen_my_share(k, gridDim.x) ? p.xw : nullptr;
#pragma unroll
    for (int i = 0; i < GR / 4; ++i) {
      const int m = wave + 4 * i, b = row0 + m;
      gen_row_put(gen_ln(gen_add4(x[0][i], x[1][i]), ln.g, ln.b, p.eps), b, p.B, keep, (long)b * GE + k, &xs[m][k]);
    }
  }
}

// ------------------------------------------------------------------ LSTM mixer gates + cell
// grid (GE / 4 unit groups, ceil(B / 16)); column n of the tile = gate n >> 2 of unit 4 bx + (n & 3)
template <int PRO>
__global__ __launch_bounds__(256) void gen_lstm_kernel(GenLstmArgs p) {
  constexpr int KP = GE + 4;
  __shared__ __attribute__((aligned(16))) float xs[GR][KP];
  __shared__ float red[4][1][GR][17];
  __shared__ float msl[GR][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * GR, u0 = 4 * blockIdx.x;
  const int n = lane & 15;
  GlW<GE> w;
  gl_wload<GE>(w, p.w_ih + (long)((n >> 2) * GE + u0 + (n & 3)) * GE, wave, lane);
  // cell thread (m, j): its unit's biases
  const int cm = tid >> 2, cj = tid & 3, cu = u0 + cj;
  float bi = 0.f, bg = 0.f, bo = 0.f;
  if (tid < 4 * GR) {
    bi = p.b_ih[cu] + p.b_hh[cu];
    bg = p.b_ih[2 * GE + cu] + p.b_hh[2 * GE + cu];
    bo = p.b_ih[3 * GE + cu] + p.b_hh[3 * GE + cu];
  }
  gen_mixer_x<PRO>(p, xs, msl);
  __syncthreads();
  gl_park(red, 0, wave, lane, gl_mma<GE>(&xs[0][0], KP, w, lane, wave));
  __syncthreads();
  if (tid < 4 * GR && row0 + cm < p.B) {
    const float zi = gl_sum(red, 0, cm, cj) + bi;
    const float zg = gl_sum(red, 0, cm, 8 + cj) + bg;
    const float zo = gl_sum(red, 0, cm, 12 + cj) + bo;
    const float c = sigmoidf_(zi) * tanhf_(zg);   // f c0 + i g with c0 = 0
    p.h[(long)(row0 + cm) * GE + cu] = sigmoidf_(zo) * tanhf_(c);
  }
}

// ------------------------------------------------------------------ GRU mixer gates + cell
// The zero-state step of torch.nn.GRU (gates r, z, n): h_0 = 0, so W_hh is never read and
// h = (1 - z) n with r = s(G_r + b_hr), z = s(G_z + b_hz), n = tanh(G_n + r b_hn), G = X W_ih^T + b_ih
// (the sums in mrg_gru_cell_fwd's order).  grid (GE / 16 unit groups, ceil(B / 16)): tile g of the
// workgroup is gate g of units 16 bx .. 16 bx + 15, weight rows g GE + 16 bx + n.
template <int PRO>
__global__ __launch_bounds__(256) void gen_gru_kernel(GenLstmArgs p) {
  constexpr int KP = GE + 4;
  __shared__ __attribute__((aligned(16))) float xs[GR][KP];
  __shared__ float red[4][3][GR][17];
  __shared__ float msl[GR][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * GR, u0 = 16 * blockIdx.x;
  GlW<GE> w[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) gl_wload<GE>(w[g], p.w_ih + (long)(g * GE + u0 + (lane & 15)) * GE, wave, lane);
  // cell thread (m, j): its unit's biases
  const int cm = tid >> 4, cj = tid & 15, cu = u0 + cj;
  const float bir = p.b_ih[cu], biz = p.b_ih[GE + cu], bin = p.b_ih[2 * GE + cu];
  const float bhr = p.b_hh[cu], bhz = p.b_hh[GE + cu], bhn = p.b_hh[2 * GE + cu];
  gen_mixer_x<PRO>(p, xs, msl);
  __syncthreads();
#pragma unroll
  for (int g = 0; g < 3; ++g) gl_park(red, g, wave, lane, gl_mma<GE>(&xs[0][0], KP, w[g], lane, wave));
  __syncthreads();
  if (row0 + cm < p.B) {
    const float rg = sigmoidf_((gl_sum(red, 0, cm, cj) + bir) + bhr);
    const float zg = sigmoidf_((gl_sum(red, 1, cm, cj) + biz) + bhz);
    const float ng = tanhf_((gl_sum(red, 2, cm, cj) + bin) + rg * bhn);
    p.h[(long)(row0 + cm) * GE + cu] = (1.0f - zg) * ng;   // + z h_0 with h_0 = 0
  }
}

// ------------------------------------------------------------------ Linear with LayerNorm prologue
// PRO 0: X = LN(a + r)                          K = 256, grid (N / 16, rows)
// PRO 1: X = LN(a2[i] + LN(a + r)), i = half     K = 256, N = 512 (two 256-column halves)
// PRO 2: X = [LN(a[0] + r[0]) | LN(a[1] + r[1])] K = 512
template <int PRO>
__global__ __launch_bounds__(256) void gen_linear_kernel(GenLinArgs p) {
  constexpr int K = PRO == 2 ? 2 * GE : GE;
  constexpr int KP = K + 4;
  constexpr int NH = PRO == 2 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float xs[GR][KP];
  __shared__ float red[4][1][GR][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * GR;
  const int n0 = 16 * blockIdx.x;
  const int half = PRO == 1 ? n0 / GE : 0;           // PRO 1: integrator of this column tile
  const int nl = n0 - half * GE;                     // first row of this half's weight
  GlW<K> w;
  gl_wload<K>(w, p.w[half] + (long)(nl + (lane & 15)) * K, wave, lane);
  const float bias = p.bias[half][nl + (tid & 15)];
  const int k = 4 * lane;
  GlLn ln[NH], ln2 = GlLn{gen_zero4(), gen_zero4()};
#pragma unroll
  for (int hh = 0; hh < NH; ++hh) ln[hh] = gl_lnp(p.ga[hh], p.be[hh], lane);
  if (PRO == 1) ln2 = gl_lnp(p.ga2[half], p.be2[half], lane);
  {
    // x[2 hh], x[2 hh + 1]: the first LayerNorm's inputs of half hh; PRO 1: x[2] the second's
    constexpr int NX = PRO == 0 ? 2 : PRO == 1 ? 3 : 4;
    const float* src[4] = {p.a[0], p.r[0], PRO == 1 ? p.a2[half] : p.a[1], p.r[1]};
    float4 x[NX][GR / 4];
    gen_rows_ld<NX>(src, p.lda, row0, p.B, wave, lane, x);
    float* keep = gen_my_share(k, PRO == 1 ? gridDim.x / 2 : gridDim.x) ? p.xw : nullptr;
#pragma unroll
    for (int i = 0; i < GR / 4; ++i) {
      const int m = wave + 4 * i, b = row0 + m;
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) {
        float4 v = gen_ln(gen_add4(x[2 * hh][i], x[2 * hh + 1][i]), ln[hh].g, ln[hh].b, p.eps);
        if (PRO == 1) v = gen_ln(gen_add4(x[2][i], v), ln2.g, ln2.b, p.eps);
        gen_row_put(v, b, p.B, keep, b * p.ldxw + half * GE + k, &xs[m][hh * GE + k]);
      }
    }
  }
  __syncthreads();
  gl_park(red, 0, wave, lane, gl_mma<K>(&xs[0][0], KP, w, lane, wave));
  __syncthreads();
  const int m = tid >> 4, nn = tid & 15, b = row0 + m;
  if (b < p.B) p.out[b * p.ldo + n0 + nn] = gl_sum(red, 0, m, nn) + bias;
}

// ------------------------------------------------------------------ FeedForward (Linear-ReLU-Linear)
// the 16 x 64 hidden rows computed per workgroup (wave w: hidden columns 16w..16w+15 over K = 256),
// then the output tile 16 x 16 over K = 64 (a k-quarter per wave).  grid (ceil(N / 16), rows).
// OUT 1: the output FeedForward's y written into pred[:, t] and the next frame's self motion
template <int PRO, int OUT>
__global__ __launch_bounds__(256) void gen_ffn_kernel(GenFfnArgs p) {
  constexpr int KP = GE + 4, HP = GHB + 4;
  __shared__ __attribute__((aligned(16))) float xs[GR][KP];
  __shared__ __attribute__((aligned(16))) float hs[GR][HP];
  __shared__ float red[4][1][GR][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * GR;
  const int n0 = 16 * blockIdx.x;
  const int hc = 16 * wave + (lane & 15);            // this lane's hidden column
  GlW<4 * GE> w1;                                    // the whole E-wide k range of the wave's own tile
  gl_wload<4 * GE>(w1, p.w1 + (long)hc * GE, 0, lane);
  const float b1 = p.b1[hc];
  const int nw = n0 + (lane & 15);
  const bool nok = nw < p.N;
  // a column past N (the output FeedForward's 6 outputs) multiplies zeroed fragments of a valid weight row
  GlW<GHB> w2;
  gl_wload<GHB>(w2, p.w2 + (long)(nok ? nw : 0) * GHB, wave, lane);
  if (!nok) w2.v[0] = gen_zero4();
  const int ocol = n0 + (tid & 15);
  const float b2 = ocol < p.N ? p.b2[ocol] : 0.0f;
  {
    GlLn ln = GlLn{gen_zero4(), gen_zero4()};
    if (PRO == 1) ln = gl_lnp(p.ga, p.be, lane);
    const float* src[2] = {p.a, p.r};
    float4 x[1 + PRO][GR / 4];
    gen_rows_ld<1 + PRO>(src, GE, row0, p.B, wave, lane, x);
#pragma unroll
    for (int i = 0; i < GR / 4; ++i) {
      const int m = wave + 4 * i;
      float4 v = x[0][i];
      if (PRO == 1) v = gen_ln(gen_add4(v, x[PRO][i]), ln.g, ln.b, p.eps);
      gen_row_put(v, row0 + m, p.B, nullptr, 0, &xs[m][4 * lane]);
    }
  }
  __syncthreads();
  {
    const gv4 acc = gl_mma<4 * GE>(&xs[0][0], KP, w1, lane, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) hs[4 * (lane >> 4) + i][hc] = fmaxf(acc[i] + b1, 0.0f);
  }
  __syncthreads();
  gl_park(red, 0, wave, lane, gl_mma<GHB>(&hs[0][0], HP, w2, lane, wave));
  __syncthreads();
  const int m = tid >> 4, nn = tid & 15, b = row0 + m;
  if (b >= p.B || ocol >= p.N) return;
  const float y = gl_sum(red, 0, m, nn) + b2;
  if (OUT == 0) {
    p.out[(long)b * p.N + ocol] = y;
  } else {
    p.pred[(long)b * p.pred_bs + (long)p.t * p.N + ocol] = y;
    const long i = (long)b * p.N + ocol;
    p.ms_next[i] = p.mask[p.t] ? y : p.ms_src[i];
  }
}

// ------------------------------------------------------------------ one query over a frame's r keys
// The audio integrator at r > 1 audio frames per prediction frame: ctx[b][h D + d] =
// sum_j softmax_j(q_h . k_hj / sqrt(D)) v_hj[d], no mask (every key of the frame is visible).
// grid (B): one workgroup per batch row, thread c owns column c, so the D lanes of a head are
// neighbours in one wave: a score is a DPP sum over 16 lanes (+ one or two cross-row shuffles at
// D = 32 / 64), every lane of the head ends with the same r scores in registers and weighs its own
// column of V.  Keys past r are loaded from key r - 1 (in bounds, no branch around a load) and
// weigh 0.  r = 1: exp(s - s) = 1 and 1 / 1 = 1, so ctx = v bitwise.
struct GenAttArgs {
  int B, r;
  const float* q;                // [B][GE]
  const float* k;                // [B][r][GE]
  const float* v;                // [B][r][GE]
  float* ctx;                    // [B][GE]
  float scale;                   // 1 / sqrt(D)
};

template <int D>
__device__ __forceinline__ float gen_head_sum(float x) {
  float s = group_sum<16>(x);
  if (D >= 32) s += __shfl_xor(s, 16);
  if (D >= 64) s += __shfl_xor(s, 32);
  return s;
}

template <int D, int RMAX>
__global__ __launch_bounds__(256) void gen_attention_kernel(GenAttArgs p) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (b >= p.B) return;
  const float* kb = p.k + (long)b * p.r * GE + c;
  const float* vb = p.v + (long)b * p.r * GE + c;
  const float q = p.q[(long)b * GE + c];
  float kk[RMAX], vv[RMAX];
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    const int jj = min(j, p.r - 1);
    kk[j] = kb[(long)jj * GE];
    vv[j] = vb[(long)jj * GE];
  }
  float s[RMAX];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    s[j] = gen_head_sum<D>(q * kk[j]) * p.scale;
    m = fmaxf(m, s[j]);   // keys past r repeat key r - 1: the maximum is that of the r keys
  }
  float e = __expf(s[0] - m);
  float sum = e, acc = e * vv[0];
#pragma unroll
  for (int j = 1; j < RMAX; ++j) {
    e = j < p.r ? __expf(s[j] - m) : 0.0f;
    sum += e;
    acc = fmaf(e, vv[j], acc);
  }
  p.ctx[(long)b * GE + c] = acc / sum;
}


// ------------------------------------------------------------------ the whole frame loop, one launch
// gen_loop_kernel runs every frame of the generation in ONE persistent launch.  Rows are independent
// (every frame is a zero-state T = 1 forward per batch row), so the batch is cut into groups of 8
// rows and each group is served by 16 workgroups that own 1/16 of every stage's output columns;
// stage outputs travel as {tag, value} granules (the recurrences' hand-off, lstm_common.h) through a
// ring the launch zeroes first, and a member polls the full rows it needs instead of waiting at a
// kernel boundary.  Members of a group share blockIdx % 8 (one XCD under the round-robin dispatch,
// checked at launch start: then the granules stay in that XCD's L2).  Full-row intermediates a
// member needs again (the block input X, Y, Y_0 / Y_1, M3) stay in its LDS.  Per block:
//   S1 gather Zf -> X = LN(Zf + M3) (block 0: ms_in W_fe^T + b_fe) -> 4 x (4 units x 4 gates) ->
//      zero-state cell -> publish h
//   S2 gather h -> Y = LN(h + X) -> Z = Y W^T + b            -> publish Z
//   S3 gather Z -> M = LN(Z + Y), Y_i = LN(a_i[t] + M) -> Z_i -> publish Z_0 | Z_1
//   S4 gather Z_0 | Z_1 -> [LN(Z_0 + Y_0) | LN(Z_1 + Y_1)] W_cat^T + b -> publish M3
//   S5 gather M3 -> relu(M3 W1^T + b1) (all 64, per member) W2^T + b2 -> publish Zf
// and after the last block every member computes the output FeedForward of its rows itself
// (LN(Zf + M3) -> 64 -> fm), so the next frame's self motion (the sampling select) needs no exchange;
// member 0 writes the prediction.  Tag of block k's buffers in frame t: t * nb + k + 1.
static constexpr int GL_NBMAX = 5;
static constexpr int GL_PER_BLOCK = 31;

struct GenLoopBlock {
  const float* p[GL_PER_BLOCK];       // see mrg_gen_loop for the order
};
struct GenLoopArgs {
  GenLoopBlock blk[GL_NBMAX];
  const float *fe_w, *fe_b, *ow1, *ob1, *ow2, *ob2;
  const float* ms;                    // [T][B][fm]
  const unsigned char* mask;          // [T]
  float* pred;                        // [B][T][fm]
  unsigned long long* ring;           // h | z | z01 | m3 | zf granules, then the XCC slots
  int* err;
  int B, T, fm, nb, ngroups;
  float eps;
  unsigned long long* stamps;         // diagnostics (mrg_gen_loop_debug_stamps): [T][16][32] of group 0, or null
};

// thread 0 of each member of row group 0: 100 MHz real-time stamp (s_memrealtime, one clock for every
// CU) `slot` of frame t into stamps[t][member][slot] (slot 31 of frame 0: the local-hand-off flag)
#define GL_STAMP(slot)                                                                   \
  do {                                                                                   \
    if (p.stamps && g == 0 && threadIdx.x == 0) {                                        \
      unsigned long long _t;                                                             \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");     \
      p.stamps[((long)t * GL_MEM + j) * 32 + (slot)] = _t;                               \
    }                                                                                    \
  } while (0)

enum { GL_WIH, GL_BIH, GL_BHH, GL_L1G, GL_L1B, GL_MW, GL_MB, GL_L2G, GL_L2B,
       GL_I0, GL_I1 = GL_I0 + 6, GL_CW = GL_I1 + 6, GL_CB, GL_FW1, GL_FB1, GL_FW2, GL_FB2, GL_FLG, GL_FLB,
       GL_ATT0, GL_ATT1 };   // integrator i: GL_Ii + {0 ln1 g, 1 ln1 b, 2 w, 3 b, 4 ln2 g, 5 ln2 b}
static_assert(GL_ATT1 + 1 == GL_PER_BLOCK, "gen loop pointer table");


__global__ __launch_bounds__(256) void gen_loop_kernel(GenLoopArgs p) {
  constexpr int XP = GE + 4, AP = 2 * GE + 4, HP = GHB + 4;
  __shared__ __attribute__((aligned(16))) float A[16][AP];      // the stage's product operand (rows 8..15 zero)
  __shared__ __attribute__((aligned(16))) float Xs[GL_ROWS][XP];
  __shared__ __attribute__((aligned(16))) float Ys[GL_ROWS][XP];
  __shared__ __attribute__((aligned(16))) float Y01[GL_ROWS][AP];
  __shared__ __attribute__((aligned(16))) float M3[GL_ROWS][XP];
  __shared__ __attribute__((aligned(16))) float hs[16][HP];
  __shared__ float red[4][4][16][17];
  __shared__ __attribute__((aligned(16))) float msin[GL_ROWS][16];
  __shared__ float fe_s[16][GE];   // feature_embedding.0 W^T (rows past fm zero) and its bias
  __shared__ float feb_s[GE];
  __shared__ int sdead, xflag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x % p.ngroups, j = blockIdx.x / p.ngroups;   // group (8 rows), member (1/16 of columns)
  const int r0 = GL_ROWS * g, B = p.B, T = p.T, fm = p.fm;
  const float eps = p.eps;
  unsigned long long* bh = p.ring;
  unsigned long long* bz = bh + (long)B * GE;
  unsigned long long* bz01 = bz + (long)B * GE;
  unsigned long long* bm3 = bz01 + (long)B * 2 * GE;
  unsigned long long* bzf = bm3 + (long)B * GE;
  unsigned long long* slots = bzf + (long)B * GE;
  bool dead = false;
  for (int i = tid; i < 16 * AP; i += 256) (&A[0][0])[i] = 0.0f;
  for (int f = 0; f < 16; ++f) fe_s[f][tid] = f < p.fm ? p.fe_w[tid * p.fm + f] : 0.0f;
  feb_s[tid] = p.fe_b[tid];
  if (tid == 0) sdead = 0;
  const int local = group_on_one_xcd<GL_MEM>(slots + (long)g * GL_MEM, j, p.err, dead, &xflag);
  if (tid < GL_ROWS * 16) {   // frame 0's self motion
    const int m = tid >> 4, f = tid & 15;
    msin[m][f] = (f < fm && r0 + m < B) ? p.ms[(long)(r0 + m) * fm + f] : 0.0f;
  }
  __syncthreads();
  const int m8 = tid >> 4, n16 = tid & 15;   // epilogue thread -> (row, column of the tile), rows < 8 used
  const bool ep = tid < GL_ROWS * 16 && r0 + m8 < B;
  const int nl = lane & 15;                  // this lane's tile column (weight row) in the products
  if (p.stamps && g == 0 && threadIdx.x == 0) p.stamps[(long)j * 32 + 31] = (unsigned long long)local;
  for (int t = 0; t < T && !sdead; ++t) {
    GL_STAMP(0);
    for (int k = 0; k < p.nb; ++k) {
      const float* const* w = p.blk[k].p;
      const unsigned tag = (unsigned)(t * p.nb + k + 1);
      // ---- S1: X, gates of units 16 j .. 16 j + 15 (tile q: units 16 j + 4 q + (n & 3), gate n >> 2), cell
      {
        GlW<GE> f[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          gl_wload<GE>(f[q], w[GL_WIH] + (long)((nl >> 2) * GE + 16 * j + 4 * q + (nl & 3)) * GE, wave, lane);
        float bi = 0.f, bg = 0.f, bo = 0.f;
        const int u = 16 * j + n16;
        if (tid < GL_ROWS * 16) {
          bi = w[GL_BIH][u] + w[GL_BHH][u];
          bg = w[GL_BIH][2 * GE + u] + w[GL_BHH][2 * GE + u];
          bo = w[GL_BIH][3 * GE + u] + w[GL_BHH][3 * GE + u];
        }
        if (k == 0) {
          // all 16 self-motion columns from LDS, unrolled (msin and fe_s are zero past fm: the same
          // sums), so the reads issue back to back instead of one round trip per column
          const int c = tid;
          float wv[16];
#pragma unroll
          for (int f = 0; f < 16; ++f) wv[f] = fe_s[f][c];
          const float bc = feb_s[c];
#pragma unroll
          for (int m = 0; m < GL_ROWS; ++m) {
            float acc = 0.0f;
#pragma unroll
            for (int f4 = 0; f4 < 4; ++f4) {
              const float4 ms4 = *reinterpret_cast<const float4*>(&msin[m][4 * f4]);
              acc = fmaf(ms4.x, wv[4 * f4], acc);
              acc = fmaf(ms4.y, wv[4 * f4 + 1], acc);
              acc = fmaf(ms4.z, wv[4 * f4 + 2], acc);
              acc = fmaf(ms4.w, wv[4 * f4 + 3], acc);
            }
            const float v = r0 + m < B ? acc + bc : 0.0f;
            Xs[m][c] = v;
            A[m][c] = v;
          }
        } else {
          const float* const* wp = p.blk[k - 1].p;
          const GlLn ln = gl_lnp(wp[GL_FLG], wp[GL_FLB], lane);
          gl_gather<GE>(bzf, r0, B, tag - 1, &A[0][0], AP, p.err, dead, &sdead);
          __syncthreads();
          for (int m = wave; m < GL_ROWS; m += 4) gl_ln_row(A[m], M3[m], ln, eps, Xs[m], A[m], lane);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) gl_park(red, q, wave, lane, gl_mma<GE>(&A[0][0], AP, f[q], lane, wave));
        __syncthreads();
        if (ep) {
          const int q = n16 >> 2, jj = n16 & 3;
          const float zi = gl_sum(red, q, m8, jj) + bi;
          const float zg = gl_sum(red, q, m8, 8 + jj) + bg;
          const float zo = gl_sum(red, q, m8, 12 + jj) + bo;
          const float c = sigmoidf_(zi) * tanhf_(zg);   // f c0 + i g with c0 = 0
          put_granule(bh + (long)(r0 + m8) * GE + u, tag, sigmoidf_(zo) * tanhf_(c), local);
        }
        GL_STAMP(1 + 5 * k);
      }
      // ---- S2: Y = LN(h + X), Z = Y W_m^T + b
      {
        GlW<GE> f;
        gl_wload<GE>(f, w[GL_MW] + (long)(16 * j + nl) * GE, wave, lane);
        const GlLn ln = gl_lnp(w[GL_L1G], w[GL_L1B], lane);
        const float bias = w[GL_MB][16 * j + n16];
        gl_gather<GE>(bh, r0, B, tag, &A[0][0], AP, p.err, dead, &sdead);
        __syncthreads();
        for (int m = wave; m < GL_ROWS; m += 4) gl_ln_row(A[m], Xs[m], ln, eps, Ys[m], A[m], lane);
        __syncthreads();
        gl_park(red, 0, wave, lane, gl_mma<GE>(&A[0][0], AP, f, lane, wave));
        __syncthreads();
        if (ep) put_granule(bz + (long)(r0 + m8) * GE + 16 * j + n16, tag, gl_sum(red, 0, m8, n16) + bias, local);
        GL_STAMP(2 + 5 * k);
      }
      // ---- S3: M = LN(Z + Y), Y_i = LN(a_i + M), Z_i = Y_i W_i^T + b_i
      {
        GlW<GE> f[2];
        GlLn l1[2];
        float bias[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          gl_wload<GE>(f[i], w[GL_I0 + 6 * i + 2] + (long)(16 * j + nl) * GE, wave, lane);
          l1[i] = gl_lnp(w[GL_I0 + 6 * i + 0], w[GL_I0 + 6 * i + 1], lane);
          bias[i] = w[GL_I0 + 6 * i + 3][16 * j + n16];
        }
        const GlLn ln = gl_lnp(w[GL_L2G], w[GL_L2B], lane);
        float4 av[2][2];   // this wave's rows' attention outputs (frame t), loaded before the poll
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            av[rr][i] = gen_ld4(w[GL_ATT0 + i] + ((long)t * B + min(r0 + wave + 4 * rr, B - 1)) * GE + 4 * lane);
        gl_gather<GE>(bz, r0, B, tag, &A[0][0], AP, p.err, dead, &sdead);
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int m = wave + 4 * rr;
          const float4 mv = gen_ln(gen_add4(*reinterpret_cast<const float4*>(&A[m][4 * lane]),
                                            *reinterpret_cast<const float4*>(&Ys[m][4 * lane])),
                                   ln.g, ln.b, eps);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const float4 y = gen_ln(gen_add4(av[rr][i], mv), l1[i].g, l1[i].b, eps);
            *reinterpret_cast<float4*>(&Y01[m][GE * i + 4 * lane]) = y;
            *reinterpret_cast<float4*>(&A[m][GE * i + 4 * lane]) = y;
          }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) gl_park(red, i, wave, lane, gl_mma<GE>(&A[0][0] + GE * i, AP, f[i], lane, wave));
        __syncthreads();
        if (ep) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
            put_granule(bz01 + (long)(r0 + m8) * 2 * GE + GE * i + 16 * j + n16, tag, gl_sum(red, i, m8, n16) + bias[i],
                        local);
        }
        GL_STAMP(3 + 5 * k);
      }
      // ---- S4: M3 = [LN(Z_0 + Y_0) | LN(Z_1 + Y_1)] W_cat^T + b
      {
        GlW<2 * GE> f;
        gl_wload<2 * GE>(f, w[GL_CW] + (long)(16 * j + nl) * 2 * GE, wave, lane);
        GlLn l2[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) l2[i] = gl_lnp(w[GL_I0 + 6 * i + 4], w[GL_I0 + 6 * i + 5], lane);
        const float bias = w[GL_CB][16 * j + n16];
        gl_gather<2 * GE>(bz01, r0, B, tag, &A[0][0], AP, p.err, dead, &sdead);
        __syncthreads();
        for (int m = wave; m < GL_ROWS; m += 4)
#pragma unroll
          for (int i = 0; i < 2; ++i) gl_ln_row(A[m] + GE * i, Y01[m] + GE * i, l2[i], eps, A[m] + GE * i, nullptr, lane);
        __syncthreads();
        gl_park(red, 0, wave, lane, gl_mma<2 * GE>(&A[0][0], AP, f, lane, wave));
        __syncthreads();
        if (ep) put_granule(bm3 + (long)(r0 + m8) * GE + 16 * j + n16, tag, gl_sum(red, 0, m8, n16) + bias, local);
        GL_STAMP(4 + 5 * k);
      }
      // ---- S5: Zf = relu(M3 W1^T + b1) W2^T + b2 (all 64 hidden columns per member, wave w: 16 w ..)
      {
        GlW<4 * GE> f1;
        gl_wload<4 * GE>(f1, w[GL_FW1] + (long)(16 * wave + nl) * GE, 0, lane);
        GlW<GHB> f2;
        gl_wload<GHB>(f2, w[GL_FW2] + (long)(16 * j + nl) * GHB, wave, lane);
        const int hc = 16 * wave + nl;
        const float b1 = w[GL_FB1][hc];
        const float bias = w[GL_FB2][16 * j + n16];
        gl_gather<GE>(bm3, r0, B, tag, &A[0][0], AP, p.err, dead, &sdead);
        __syncthreads();
        for (int i = tid; i < GL_ROWS * GE; i += 256) M3[i / GE][i % GE] = A[i / GE][i % GE];
        {
          const gv4 acc = gl_mma<4 * GE>(&A[0][0], AP, f1, lane, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) hs[4 * (lane >> 4) + i][hc] = fmaxf(acc[i] + b1, 0.0f);
        }
        __syncthreads();
        gl_park(red, 0, wave, lane, gl_mma<GHB>(&hs[0][0], HP, f2, lane, wave));
        __syncthreads();
        if (ep) put_granule(bzf + (long)(r0 + m8) * GE + 16 * j + n16, tag, gl_sum(red, 0, m8, n16) + bias, local);
        GL_STAMP(5 + 5 * k);
      }
    }
    // ---- output FeedForward of this group's rows (every member), the sampling select
    {
      const float* const* wl = p.blk[p.nb - 1].p;
      GlW<4 * GE> f1;
      gl_wload<4 * GE>(f1, p.ow1 + (long)(16 * wave + nl) * GE, 0, lane);
      // columns past fm multiply zeroed fragments of a clamped (valid) weight row
      GlW<GHB> f2;
      gl_wload<GHB>(f2, p.ow2 + (long)(nl < fm ? nl : 0) * GHB, wave, lane);
      if (nl >= fm) f2.v[0] = make_float4(0.f, 0.f, 0.f, 0.f);
      const GlLn ln = gl_lnp(wl[GL_FLG], wl[GL_FLB], lane);
      const int hc = 16 * wave + nl;
      const float b1 = p.ob1[hc];
      const float b2 = n16 < fm ? p.ob2[n16] : 0.0f;
      gl_gather<GE>(bzf, r0, B, (unsigned)(t * p.nb + p.nb), &A[0][0], AP, p.err, dead, &sdead);
      __syncthreads();
      for (int m = wave; m < GL_ROWS; m += 4) gl_ln_row(A[m], M3[m], ln, eps, A[m], nullptr, lane);
      __syncthreads();
      {
        const gv4 acc = gl_mma<4 * GE>(&A[0][0], AP, f1, lane, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) hs[4 * (lane >> 4) + i][hc] = fmaxf(acc[i] + b1, 0.0f);
      }
      __syncthreads();
      gl_park(red, 0, wave, lane, gl_mma<GHB>(&hs[0][0], HP, f2, lane, wave));
      __syncthreads();
      if (tid < GL_ROWS * 16) {
        const int b = r0 + m8;
        float nxt = 0.0f;
        if (n16 < fm && b < B) {
          const float y = gl_sum(red, 0, m8, n16) + b2;
          if (j == 0) p.pred[((long)b * T + t) * fm + n16] = y;
          nxt = p.mask[t] ? y : p.ms[((long)t * B + b) * fm + n16];
        }
        msin[m8][n16] = nxt;
      }
      if (dead) sdead = 1;
      __syncthreads();
      GL_STAMP(30);
    }
  }
}

}  // namespace mrg

using namespace mrg;

static int gen_rows(int B) { return (B + GR - 1) / GR; }

// The recurrent mixers' launch: X [B][256] from the self-motion input (block 0: ms W_fe^T + b_fe,
// fm <= 16) or from the previous block's FeedForward (LN(a + r)) into xw, then the mixer's zero-state step
// -> h [B][256].  `units`: the units a workgroup's column tiles serve.
template <typename Kern>
static int gen_mixer_launch(const char* name, Kern from_ms, Kern from_ln, int units, const GenLstmArgs& p,
                            hipStream_t stream) {
  if (p.B == 0) return 0;
  MRG_REQUIRE(p.B > 0 && p.xw && p.w_ih && p.b_ih && p.b_hh && p.h, "%s: B >= 0 and xw / w_ih / b_ih / b_hh / h (B=%d)",
              name, p.B);
  MRG_REQUIRE(!(p.ms && (p.a || p.r || p.ga || p.be)), "%s: give ms or the LayerNorm inputs, not both", name);
  MRG_REQUIRE(p.ms ? (p.fm >= 1 && p.fm <= 16 && p.fe_w && p.fe_b) : (p.a && p.r && p.ga && p.be),
              "%s: give ms + feature embedding (fm <= 16) or the LayerNorm inputs (fm=%d)", name, p.fm);
  klaunch(p.ms ? from_ms : from_ln, dim3(GE / units, gen_rows(p.B)), 256, 0, stream, p);
  return check_launch(name);
}

// The LSTM mixer: gates = X W_ih^T + b_ih + b_hh (w_ih [1024][256], gates i, f, g, o), zero-state cell.
MRG_API int mrg_gen_lstm(int B, int fm, const float* ms, const float* fe_w, const float* fe_b, const float* a,
                         const float* r, const float* ga, const float* be, float eps, float* xw, const float* w_ih,
                         const float* b_ih, const float* b_hh, float* h, hipStream_t stream) {
  return gen_mixer_launch("mrg_gen_lstm", gen_lstm_kernel<0>, gen_lstm_kernel<1>, 4,
                          {B, fm, ms, fe_w, fe_b, a, r, ga, be, eps, xw, w_ih, b_ih, b_hh, h}, stream);
}

// The GRU mixer: the zero-state torch.nn.GRU step (gates r, z, n; w_ih [768][256], b_ih / b_hh [768];
// W_hh is not read).
MRG_API int mrg_gen_gru(int B, int fm, const float* ms, const float* fe_w, const float* fe_b, const float* a,
                        const float* r, const float* ga, const float* be, float eps, float* xw, const float* w_ih,
                        const float* b_ih, const float* b_hh, float* h, hipStream_t stream) {
  return gen_mixer_launch("mrg_gen_gru", gen_gru_kernel<0>, gen_gru_kernel<1>, 16,
                          {B, fm, ms, fe_w, fe_b, a, r, ga, be, eps, xw, w_ih, b_ih, b_hh, h}, stream);
}

// mode 0: out [B][256] = LN(a + r) W^T + b, the normalised rows into xw [B][256]
// mode 1: the two integrators: M = LN(a + r) (ga[0]), Y_i = LN(a2[i] + M) (ga2[i]) into xw[:, 256 i:],
//         out[:, 256 i:] = Y_i W_i^T + b_i   (out, xw [B][512])
// mode 2: out [B][256] = [LN(a[0] + r[0]) | LN(a[1] + r[1])] W^T + b   (W [256][512]; a, r of stride lda)
MRG_API int mrg_gen_linear(int mode, int B, const float* const* a, const float* const* r, const float* const* ga,
                           const float* const* be, long lda, const float* const* a2, const float* const* ga2,
                           const float* const* be2, float eps, float* xw, long ldxw, const float* const* w,
                           const float* const* bias, float* out, long ldo, hipStream_t stream) {
  if (B == 0) return 0;
  MRG_REQUIRE(mode >= 0 && mode <= 2 && a && r && ga && be && w && bias && out,
              "mrg_gen_linear: bad arguments (mode %d)", mode);
  GenLinArgs p{};
  p.B = B;
  const int nh = mode == 0 ? 1 : 2;
  for (int i = 0; i < 2; ++i) {
    const int s = (mode == 2 && i < nh) ? i : 0;
    p.a[i] = a[s]; p.r[i] = r[s]; p.ga[i] = ga[s]; p.be[i] = be[s];
    const int t = (mode == 1) ? i : 0;
    p.w[i] = w[t]; p.bias[i] = bias[t];
    if (mode == 1) {
      MRG_REQUIRE(a2 && ga2 && be2, "mrg_gen_linear: mode 1 needs the second LayerNorm's inputs");
      p.a2[i] = a2[i]; p.ga2[i] = ga2[i]; p.be2[i] = be2[i];
    }
  }
  p.lda = lda; p.eps = eps; p.xw = xw; p.ldxw = ldxw; p.out = out; p.ldo = ldo;
  const dim3 grid(mode == 1 ? 2 * GE / 16 : GE / 16, gen_rows(B));
  if (mode == 0) klaunch(gen_linear_kernel<0>, grid, 256, 0, stream, p);
  else if (mode == 1) klaunch(gen_linear_kernel<1>, grid, 256, 0, stream, p);
  else klaunch(gen_linear_kernel<2>, grid, 256, 0, stream, p);
  return check_launch("gen_linear_kernel");
}

// FeedForward 256 -> 64 -> ReLU -> N of X = a (r null) or LN(a + r).  pred null: out [B][N] (N = 256).
// pred given (the output FeedForward, N <= 16): y into pred[b * pred_bs + t * N + n] and
// ms_next [B][N] = mask[t] ? y : ms_src (the next frame's self motion, lstmformer.py:487-492).
MRG_API int mrg_gen_ffn(int B, int N, const float* a, const float* r, const float* ga, const float* be, float eps,
                        const float* w1, const float* b1, const float* w2, const float* b2, float* out, float* pred,
                        long pred_bs, float* ms_next, const float* ms_src, const unsigned char* mask, int t,
                        hipStream_t stream) {
  if (B == 0) return 0;
  MRG_REQUIRE(a && w1 && b1 && w2 && b2 && (r == nullptr || (ga && be)), "mrg_gen_ffn: bad arguments");
  MRG_REQUIRE(pred ? (N >= 1 && N <= 16 && ms_next && ms_src && mask) : (N == GE && out),
              "mrg_gen_ffn: N = 256 with out, or N <= 16 with pred / ms_next / ms_src / mask (N=%d)", N);
  GenFfnArgs p{B, N, a, r, ga, be, eps, w1, b1, w2, b2, out, pred, pred_bs, ms_next, ms_src, mask, t};
  const dim3 grid((N + 15) / 16, gen_rows(B));
  if (r && pred) klaunch(gen_ffn_kernel<1, 1>, grid, 256, 0, stream, p);
  else if (r) klaunch(gen_ffn_kernel<1, 0>, grid, 256, 0, stream, p);
  else if (pred) klaunch(gen_ffn_kernel<0, 1>, grid, 256, 0, stream, p);
  else klaunch(gen_ffn_kernel<0, 0>, grid, 256, 0, stream, p);
  return check_launch("gen_ffn_kernel");
}

// ctx [B][256] = the attention of one query row q [B][256] (projected, bias added) over this frame's r
// projected keys / values k, v [B][r][256], `heads` heads of D = 256 / heads in {16, 32, 64}
// concatenated, scores scaled by 1 / sqrt(D), no mask; 1 <= r <= 16.
MRG_API int mrg_gen_attention(int B, int r, int heads, const float* q, const float* k, const float* v, float* ctx,
                              hipStream_t stream) {
  MRG_REQUIRE(B >= 0 && r >= 1 && r <= 16, "mrg_gen_attention: B >= 0 and 1 <= r <= 16 (B=%d r=%d)", B, r);
  MRG_REQUIRE(heads == 4 || heads == 8 || heads == 16, "mrg_gen_attention: heads must be 4, 8 or 16 (heads=%d)", heads);
  if (B == 0) return 0;
  MRG_REQUIRE(q && k && v && ctx, "mrg_gen_attention: null buffer");
  const int D = GE / heads;
  GenAttArgs p{B, r, q, k, v, ctx, 1.0f / sqrtf((float)D)};
  const dim3 grid(B);
#define MRG_GEN_ATT(DD)                                                                   \
  do {                                                                                    \
    if (r <= 4) klaunch(gen_attention_kernel<DD, 4>, grid, 256, 0, stream, p);            \
    else if (r <= 8) klaunch(gen_attention_kernel<DD, 8>, grid, 256, 0, stream, p);       \
    else klaunch(gen_attention_kernel<DD, 16>, grid, 256, 0, stream, p);                  \
  } while (0)
  if (D == 64) MRG_GEN_ATT(64);
  else if (D == 32) MRG_GEN_ATT(32);
  else MRG_GEN_ATT(16);
#undef MRG_GEN_ATT
  return check_launch("gen_attention_kernel");
}

static unsigned long long* g_gen_stamps = nullptr;
// Diagnostics (tools/gen_stamps.py): later mrg_gen_loop launches write row group 0's members' per-stage
// real-time (10 ns) stamps into buf ([T][16 members][32] u64; slot 31 of frame 0: the local hand-off
// flag); null = off.
MRG_API int mrg_gen_loop_debug_stamps(void* buf) {
  g_gen_stamps = static_cast<unsigned long long*>(buf);
  return 0;
}

// Bytes of the granule ring mrg_gen_loop needs (zeroed by the caller before every launch).
MRG_API long mrg_gen_loop_ring_bytes(int B) {
  const int ng = (B + GL_ROWS - 1) / GL_ROWS;
  return ((long)B * 6 * GE + (long)ng * GL_MEM) * 8;
}

// 1 when the whole persistent grid (16 workgroups per 8 batch rows) can be resident on `cus` CUs.
MRG_API int mrg_gen_loop_fits(int B, int cus) {
  const long nblk = (long)GL_MEM * ((B + GL_ROWS - 1) / GL_ROWS);
  return fits(gen_loop_kernel, 256, nblk, cus > 0 ? cus : device_cus()) ? 1 : 0;
}

// The whole generation frame loop in one persistent launch (gen_loop_kernel above): nb <= 5 blocks.
// ptrs (host array, 31 nb + 6 device pointers): per block w_ih, b_ih, b_hh, ln1 g / b (mixer
// LayerNorm), mixer Linear w / b, ln2 g / b (the mixer FeedForward's LayerNorm), per integrator i
// (ln1 g / b of the attention residual, FeedForward w / b, ln2 g / b), cat_linear w / b, block
// FeedForward w1 / b1 / w2 / b2, its LayerNorm g / b, the integrators' attention outputs a_0 / a_1
// [T][B][256]; then feature_embedding.0 w / b and the output FeedForward w1 / b1 / w2 / b2.
// ms [T][B][fm] (padding zeroed), mask [T] bytes, pred [B][T][fm]; ring: mrg_gen_loop_ring_bytes of
// zeroed memory; err: the recurrences' error flag (a hand-off poll that times out sets it).
MRG_API int mrg_gen_loop(int B, int T, int fm, int nb, float eps, const void* const* ptrs, int nptrs, const float* ms,
                         const unsigned char* mask, float* pred, void* ring, int* err, hipStream_t stream) {
  if (B == 0 || T == 0) return 0;
  MRG_REQUIRE(nb >= 1 && nb <= GL_NBMAX && nptrs == GL_PER_BLOCK * nb + 6 && fm >= 1 && fm <= 16 && ptrs && ms &&
                  mask && pred && ring && err,
              "mrg_gen_loop: bad arguments (B=%d nb=%d fm=%d nptrs=%d)", B, nb, fm, nptrs);
  MRG_REQUIRE(mrg_gen_loop_fits(B, 0) == 1, "mrg_gen_loop: %d workgroups cannot all be resident (B=%d)",
              GL_MEM * ((B + GL_ROWS - 1) / GL_ROWS), B);
  GenLoopArgs a{};
  for (int k = 0; k < nb; ++k)
    for (int i = 0; i < GL_PER_BLOCK; ++i) {
      a.blk[k].p[i] = static_cast<const float*>(ptrs[k * GL_PER_BLOCK + i]);
      MRG_REQUIRE(a.blk[k].p[i] != nullptr, "mrg_gen_loop: null pointer %d of block %d", i, k);
    }
  const float* const* gp = reinterpret_cast<const float* const*>(ptrs + GL_PER_BLOCK * nb);
  a.fe_w = gp[0]; a.fe_b = gp[1]; a.ow1 = gp[2]; a.ob1 = gp[3]; a.ow2 = gp[4]; a.ob2 = gp[5];
  a.ms = ms; a.mask = mask; a.pred = pred; a.ring = static_cast<unsigned long long*>(ring); a.err = err;
  a.B = B; a.T = T; a.fm = fm; a.nb = nb; a.ngroups = (B + GL_ROWS - 1) / GL_ROWS; a.eps = eps;
  a.stamps = g_gen_stamps;
  klaunch(gen_loop_kernel, dim3(GL_MEM * a.ngroups), 256, 0, stream, a);
  return check_launch("gen_loop_kernel");
}
