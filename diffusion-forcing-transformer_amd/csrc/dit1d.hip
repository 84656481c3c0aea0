// DiT1D backbone (the frame-causal transformer over 1-D token latents: TiTok-KL [C, 1, L] frames) on MI355X.
// Mirrors the module tree / state-dict names of the reference (algorithms/dfot/backbones/dit1d/dit_model.py:358-530) at the stock
// dit1d.yaml: merge_mode share_norm, causal_attn_mode video_temporal_causal (or null), no rotary embedding, no qk-norm, no context.
//
// Layout: tokens are rows [B][T*L][hidden]; the residual stream X is fp32, GEMM operands bf16.
// Conditioning: t = MLP([cos | sin](level)) depends on the integer level only and every block consumes it through Linear(SiLU(t)), so
// finalize() evaluates the six modulations of every block for every level with one GEMM into mod_table[level][depth * 6 * hidden]
// (the DiT3D engine's scheme, dit.hip); forward indexes it per frame.
//
// A block under share_norm (dit_model.py:248-271) OVERWRITES the residual stream with its LayerNorm:
//     x = LN(x);  x = x + gate_msa * attn(x * (1 + scale_msa) + shift_msa);  x = LN(x);  x = x + gate_mlp * mlp(x * (1 + scale_mlp) + shift_mlp)
// ln_share_kernel writes both the normalised row (fp32, the new residual base, in place) and its modulated bf16 copy (the GEMM operand);
// the gated GEMM epilogue then adds onto the normalised row.
#include <cmath>
#include <string>
#include <vector>

#include "dfot_hip.h"
#include "dit1d_train.h"
#include "engine_device.h"
#include "gemm.h"
#include "kernels.h"
#include "level_embed.h"

namespace dfot {
namespace {

typedef __attribute__((ext_vector_type(4))) float float4v;
constexpr int D1_FREQ = 256;     // TimestepEmbedder.frequency_embedding_size
constexpr int D1_MAX_CHUNKS = 8; // float4 chunks per lane of a row: hidden <= 2048

struct D1Block {
  bf16 *w_qkv = nullptr, *w_proj = nullptr, *w_fc1 = nullptr, *w_fc2 = nullptr;
  float *b_qkv = nullptr, *b_proj = nullptr, *b_fc1 = nullptr, *b_fc2 = nullptr;
  long mod = 0;  // column of this block's (shift_msa|scale_msa|gate_msa|shift_mlp|scale_mlp|gate_mlp) inside a mod_table row
};

__global__ void d1_clamp_levels_kernel(const int* __restrict__ levels, int* __restrict__ idx, int n, int max_level) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int lv = levels[i];
  idx[i] = lv < 0 ? 0 : (lv > max_level ? max_level : lv);
}

// Token embedding (dit_model.py:501-512): X[(b, t*L + l)][:] = W x[b][t][:][0][l] + bias + pos_embed[t*L + l].  A frame is channel-major,
// so a token's C values sit L floats apart.  One thread per 4 output channels of a token, looping over the C <= 64 channels.
__global__ __launch_bounds__(256) void d1_tok_embed_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, const float* __restrict__ pos,
                                                           float* __restrict__ X, int C, int L, int n, int hidden, long total4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int h4 = hidden / 4;
  const int c4 = (int)(i % h4) * 4;
  const long row = i / h4;       // (video, token)
  const int tok = (int)(row % n);
  const long frame = row / L;    // (video, frame): n is a whole number of frames
  const int l = tok % L;
  const float* xf = x + frame * C * L + l;
  float4v acc = *reinterpret_cast<const float4v*>(b + c4);
  for (int c = 0; c < C; ++c) {
    const float xv = xf[(long)c * L];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += w[(long)(c4 + j) * C + c] * xv;
  }
  acc += *reinterpret_cast<const float4v*>(pos + (long)tok * hidden + c4);
  *reinterpret_cast<float4v*>(X + row * hidden + c4) = acc;
}

// one wave per row: v[i] <- (x - mean) * rstd of channels (i*64 + lane)*4 .. +3 (chunks at or past hidden stay untouched)
__device__ __forceinline__ void d1_ln_row(const float* __restrict__ xr, int hidden, float eps, int lane, float4v (&v)[D1_MAX_CHUNKS]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = float4v{0.f, 0.f, 0.f, 0.f};
    if (c < hidden) v[i] = *reinterpret_cast<const float4v*>(xr + c);
    s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  }
  const float mean = wave_sum(s) / (float)hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < hidden) {
      v[i] -= mean;
      q += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)hidden + eps);
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) v[i] *= rstd;
}

// share_norm LayerNorm: X[row] <- LN(X[row]) (fp32, in place: the block's new residual base), A[row] <- bf16(LN * (1 + scale) + shift)
// with (shift | scale) = table[idx[row / rows_per_frame]][off .. off + 2 hidden)
__global__ __launch_bounds__(256) void d1_ln_share_kernel(float* __restrict__ X, bf16* __restrict__ A, const float* __restrict__ table,
                                                          const int* __restrict__ idx, long ldt, long off, int hidden,
                                                          int rows_per_frame, int rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4v v[D1_MAX_CHUNKS];
  float* xr = X + (long)row * hidden;
  d1_ln_row(xr, hidden, eps, lane, v);
  const float* sh = table + (long)idx[row / rows_per_frame] * ldt + off;
  const float* sc = sh + hidden;
  bf16* ar = A + (long)row * hidden;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < hidden) {
      *reinterpret_cast<float4v*>(xr + c) = v[i];
      const float4v a = *reinterpret_cast<const float4v*>(sh + c);
      const float4v g = *reinterpret_cast<const float4v*>(sc + c);
      const float4v m = v[i] * (1.0f + g) + a;
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bf(m[j]);
      *reinterpret_cast<bf16x4*>(ar + c) = o;
    }
  }
}

// Final layer (dit_model.py:453-456, 524-530): LayerNorm (no affine) -> Linear(hidden, C), written straight into (B, T, C, 1, L):
// token (frame, l), channel c -> out[(frame * C + c) * L + l].  One wave per token row.
__global__ __launch_bounds__(256) void d1_final_kernel(const float* __restrict__ X, const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ out, int hidden, int C, int L, int rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4v v[D1_MAX_CHUNKS];
  d1_ln_row(X + (long)row * hidden, hidden, eps, lane, v);
  const long frame = row / L;
  const int l = row % L;
  for (int c = 0; c < C; ++c) {
    const float* wr = w + (long)c * hidden;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
      const int ch = (i * 64 + lane) * 4;
      if (ch < hidden) {
        const float4v ww = *reinterpret_cast<const float4v*>(wr + ch);
        acc += (v[i][0] * ww[0] + v[i][1] * ww[1]) + (v[i][2] * ww[2] + v[i][3] * ww[3]);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) out[(frame * C + c) * L + l] = acc + b[c];
  }
}

// ---- the launches of the kernels above: each exists once, for the engine's forward and for the dfot_op_dit1d_* entries ----
int launch_d1_clamp_levels(const int* levels, int* idx, int frames, int max_level, hipStream_t s) {
  hipLaunchKernelGGL(d1_clamp_levels_kernel, dim3(cdiv(frames, 256)), dim3(256), 0, s, levels, idx, frames, max_level);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
// x [frames][C][L] -> X [rows][hidden], rows = videos * n tokens, n a whole number of L-token frames; pos [n][hidden]
int launch_d1_tok_embed(const float* x, const float* w, const float* b, const float* pos, float* X, int C, int L, int n, int hidden, long rows,
                        hipStream_t s) {
  const long total4 = rows * (hidden / 4);
  hipLaunchKernelGGL(d1_tok_embed_kernel, dim3(cdiv(total4, 256)), dim3(256), 0, s, x, w, b, pos, X, C, L, n, hidden, total4);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
int launch_d1_ln_share(float* X, bf16* A, const float* table, const int* idx, long ldt, long off, int hidden, int rows_per_frame, int rows, float eps,
                       hipStream_t s) {
  hipLaunchKernelGGL(d1_ln_share_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, X, A, table, idx, ldt, off, hidden, rows_per_frame, rows, eps);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
int launch_d1_final(const float* X, const float* w, const float* b, float* out, int hidden, int C, int L, int rows, float eps, hipStream_t s) {
  hipLaunchKernelGGL(d1_final_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, X, w, b, out, hidden, C, L, rows, eps);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace

// the two ends of the forward for the training engine (dit1d_train.inl, another translation unit; declared in dit1d_train.h)
int d1_tok_embed(const float* x, const float* w, const float* b, const float* pos, float* X, int C, int L, int n, int hidden, long rows,
                 hipStream_t s) {
  return launch_d1_tok_embed(x, w, b, pos, X, C, L, n, hidden, rows, s);
}
int d1_final(const float* X, const float* w, const float* b, float* out, int hidden, int C, int L, int rows, float eps, hipStream_t s) {
  return launch_d1_final(X, w, b, out, hidden, C, L, rows, eps, s);
}

}  // namespace dfot

using namespace dfot;

struct dfot_dit1d_s : EngineDevice {
  dfot_dit1d_s() : EngineDevice("dit1d ") {}
  dfot_dit1d_config cfg{};
  int d = 0, dstride = 0, lpad = 0, ntok = 0;  // head dim, q/k/v row stride, level count padded to the GEMM row tile, T * L
  long ldt = 0;                                // mod_table row: depth * 6 * hidden
  // weights
  float *pos = nullptr, *x_w = nullptr, *x_b = nullptr, *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr,
        *fin_w = nullptr, *fin_b = nullptr, *b_mod = nullptr;
  bf16* w_mod = nullptr;  // every adaLN_modulation.1 stacked: [ldt][hidden]
  std::vector<D1Block> blocks;
  // derived at finalize
  float *freqs = nullptr, *feat = nullptr, *thid = nullptr, *mod_table = nullptr;
  bf16* semb = nullptr;
  bool finalized = false;
  // workspace
  int max_batch = 0;
  float* X = nullptr;
  bf16 *A = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *hid = nullptr;
  int* idx = nullptr;
};

namespace dfot {
namespace {

int d1_build(dfot_dit1d_s* h) {
  const dfot_dit1d_config& c = h->cfg;
  const int hd = c.hidden, mh = c.mlp_hidden;
  h->d = hd / c.heads;
  h->dstride = attention_dstride(h->d);
  h->ntok = c.max_tokens * c.tokens_per_frame;
  h->ldt = (long)c.depth * 6 * hd;
  h->lpad = (c.timesteps + 255) / 256 * 256;
  int rc = 0;
  if ((rc = h->alloc(&h->w_mod, (size_t)h->ldt * hd)) || (rc = h->alloc(&h->b_mod, (size_t)h->ldt))) return rc;
  h->blocks.resize(c.depth);
  // registration order == the reference module's state_dict order
  if ((rc = h->add_f32("pos_embed", {1, h->ntok, hd}, &h->pos))) return rc;
  if ((rc = h->add_f32("x_embedder.weight", {hd, c.in_channels}, &h->x_w)) || (rc = h->add_f32("x_embedder.bias", {hd}, &h->x_b))) return rc;
  if ((rc = h->add_f32("t_embedder.mlp.0.weight", {hd, D1_FREQ}, &h->t_w1)) || (rc = h->add_f32("t_embedder.mlp.0.bias", {hd}, &h->t_b1)) ||
      (rc = h->add_f32("t_embedder.mlp.2.weight", {hd, hd}, &h->t_w2)) || (rc = h->add_f32("t_embedder.mlp.2.bias", {hd}, &h->t_b2)))
    return rc;
  for (int i = 0; i < c.depth; ++i) {
    D1Block& w = h->blocks[i];
    const std::string p = "blocks." + std::to_string(i) + ".";
    w.mod = (long)i * 6 * hd;
    if ((rc = h->add_linear(p + "attn.qkv.weight", 3 * hd, hd, &w.w_qkv)) || (rc = h->add_f32(p + "attn.qkv.bias", {3 * hd}, &w.b_qkv)) ||
        (rc = h->add_linear(p + "attn.proj.weight", hd, hd, &w.w_proj)) || (rc = h->add_f32(p + "attn.proj.bias", {hd}, &w.b_proj)) ||
        (rc = h->add_linear(p + "mlp.fc1.weight", mh, hd, &w.w_fc1)) || (rc = h->add_f32(p + "mlp.fc1.bias", {mh}, &w.b_fc1)) ||
        (rc = h->add_linear(p + "mlp.fc2.weight", hd, mh, &w.w_fc2)) || (rc = h->add_f32(p + "mlp.fc2.bias", {hd}, &w.b_fc2)))
      return rc;
    h->add_bf16(p + "adaLN_modulation.1.weight", 6 * hd, hd, h->w_mod + w.mod * hd);
    h->add_slice(p + "adaLN_modulation.1.bias", {6 * hd}, h->b_mod + w.mod);
  }
  if ((rc = h->add_f32("final_layer.1.weight", {c.in_channels, hd}, &h->fin_w)) ||
      (rc = h->add_f32("final_layer.1.bias", {c.in_channels}, &h->fin_b)))
    return rc;

  std::vector<float> freqs(D1_FREQ / 2);
  for (int i = 0; i < D1_FREQ / 2; ++i)  // torch.exp(-math.log(10000) * arange(half, dtype=float32) / half): fp32 throughout
    freqs[i] = expf((float)(-std::log(10000.0)) * (float)i / (float)(D1_FREQ / 2));
  if ((rc = h->alloc(&h->freqs, freqs.size()))) return rc;
  DFOT_CHECK_HIP(hipMemcpy(h->freqs, freqs.data(), freqs.size() * sizeof(float), hipMemcpyHostToDevice));
  if ((rc = h->alloc(&h->feat, (size_t)h->lpad * D1_FREQ)) || (rc = h->alloc(&h->thid, (size_t)h->lpad * hd)) ||
      (rc = h->alloc(&h->semb, (size_t)h->lpad * hd)) ||
      (rc = h->alloc(&h->mod_table, (size_t)h->lpad * h->ldt)))
    return rc;
  return DFOT_OK;
}

}  // namespace
}  // namespace dfot

extern "C" {

int dfot_dit1d_destroy(dfot_dit1d_t h) {
  if (!h) return DFOT_OK;
  h->free_all();
  delete h;
  return DFOT_OK;
}

int dfot_dit1d_create(const dfot_dit1d_config* cfg, dfot_dit1d_t* out) {
  DFOT_REQUIRE(cfg && out, DFOT_ERR_ARG, "dfot_dit1d_create: null argument");
  const dfot_dit1d_config& c = *cfg;
  DFOT_REQUIRE(c.hidden > 0 && c.hidden % 64 == 0 && c.hidden <= 2048, DFOT_ERR_SHAPE, "dit1d: hidden %d must be a multiple of 64, <= 2048", c.hidden);
  DFOT_REQUIRE(c.heads > 0 && c.hidden % c.heads == 0, DFOT_ERR_SHAPE, "dit1d: hidden %d not divisible by %d heads", c.hidden, c.heads);
  const int d = c.hidden / c.heads;
  DFOT_REQUIRE(d % 8 == 0 && d <= 128, DFOT_ERR_SHAPE, "dit1d: head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(c.mlp_hidden > 0 && c.mlp_hidden % 64 == 0, DFOT_ERR_SHAPE, "dit1d: mlp_hidden %d must be a positive multiple of 64", c.mlp_hidden);
  DFOT_REQUIRE(c.in_channels > 0 && c.in_channels <= 64, DFOT_ERR_SHAPE, "dit1d: in_channels %d must be in [1, 64]", c.in_channels);
  const int L = c.tokens_per_frame;
  DFOT_REQUIRE(L == 16 || L == 32 || L == 64 || L == 128, DFOT_ERR_SHAPE, "dit1d: tokens_per_frame %d not in {16, 32, 64, 128}", L);
  DFOT_REQUIRE(c.max_tokens > 0 && ((long)c.max_tokens * L) % 128 == 0 && (long)c.max_tokens * L <= (1 << 20), DFOT_ERR_SHAPE,
               "dit1d: max_tokens %d x tokens_per_frame %d must be a multiple of 128", c.max_tokens, L);
  DFOT_REQUIRE(c.depth > 0 && c.timesteps > 0, DFOT_ERR_SHAPE, "dit1d: bad depth %d / timesteps %d", c.depth, c.timesteps);
  DFOT_REQUIRE(c.causal == 0 || c.causal == 1, DFOT_ERR_ARG, "dit1d: causal %d must be 0 or 1", c.causal);
  DFOT_REQUIRE(c.eps > 0.f, DFOT_ERR_ARG, "dit1d: eps must be positive");
  auto* h = new dfot_dit1d_s();
  h->cfg = c;
  int rc = d1_build(h);
  if (rc) {
    dfot_dit1d_destroy(h);
    return rc;
  }
  *out = h;
  return DFOT_OK;
}

int dfot_dit1d_num_params(dfot_dit1d_t h) { return h ? h->params.count() : 0; }
const char* dfot_dit1d_param_name(dfot_dit1d_t h, int i) { return h ? h->params.name(i) : nullptr; }
int dfot_dit1d_param_shape(dfot_dit1d_t h, int i, int64_t shape[4], int* ndim) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "dit1d param_shape: bad argument");
  return h->params.shape(i, shape, ndim);
}

int dfot_dit1d_load_weight(dfot_dit1d_t h, const char* name, const float* data, const int64_t* shape, int ndim, void* stream) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "dit1d load_weight: null argument");
  int rc = h->params.load(name, data, shape, ndim, (hipStream_t)stream);
  if (!rc) h->finalized = false;
  return rc;
}

int dfot_dit1d_finalize(dfot_dit1d_t h, void* stream) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "dit1d finalize: null handle");
  int rc = h->params.require_all_loaded();
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dfot_dit1d_config& c = h->cfg;
  const int hd = c.hidden, Lv = c.timesteps;
  // embedding of every level: [cos | sin] -> Linear -> SiLU -> Linear (t) ; semb = bf16(SiLU(t)) feeds every adaLN_modulation
  hipLaunchKernelGGL(tstep_features_kernel, dim3(cdiv((long)Lv * D1_FREQ, 256)), dim3(256), 0, s, h->freqs, h->feat, Lv, D1_FREQ);
  DFOT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rows_linear_kernel<1>, dim3(cdiv(hd, 4), Lv), dim3(256), 0, s, h->feat, h->t_w1, h->t_b1, h->thid, (bf16*)nullptr,
                     D1_FREQ, hd);
  DFOT_CHECK_HIP(hipGetLastError());
  DFOT_CHECK_HIP(hipMemsetAsync(h->semb, 0, (size_t)h->lpad * hd * sizeof(bf16), s));
  hipLaunchKernelGGL(rows_linear_kernel<0>, dim3(cdiv(hd, 4), Lv), dim3(256), 0, s, h->thid, h->t_w2, h->t_b2, (float*)nullptr, h->semb, hd, hd);
  DFOT_CHECK_HIP(hipGetLastError());
  GemmArgs g;
  g.A = h->semb; g.lda = hd; g.W = h->w_mod; g.M = h->lpad; g.N = (int)h->ldt; g.K = hd;
  g.bias = h->b_mod; g.out_f32 = h->mod_table; g.ldo = h->ldt;
  if ((rc = launch_gemm(A_DENSE, E_F32, gemm_pick_variant(A_DENSE, g.M, g.N, g.K, true), g, s))) return rc;
  DFOT_CHECK_HIP(hipStreamSynchronize(s));
  h->finalized = true;
  return DFOT_OK;
}

int dfot_dit1d_reserve(dfot_dit1d_t h, int max_batch) {
  DFOT_REQUIRE(h && max_batch > 0, DFOT_ERR_ARG, "dit1d reserve: bad argument");
  if (max_batch <= h->max_batch) return DFOT_OK;
  h->free_workspace();
  h->max_batch = 0;
  const dfot_dit1d_config& c = h->cfg;
  const size_t rows = (size_t)max_batch * h->ntok;
  const size_t qkv = (size_t)max_batch * c.heads * h->ntok * h->dstride;
  int rc = 0;
  if ((rc = h->alloc(&h->X, rows * c.hidden, true)) || (rc = h->alloc(&h->A, rows * c.hidden, true))) return rc;
  if ((rc = h->alloc(&h->q, qkv, true)) || (rc = h->alloc(&h->k, qkv, true)) || (rc = h->alloc(&h->v, qkv, true))) return rc;
  // pad columns d..dstride of q/k/v are never written by the QKV epilogue: zero them once
  DFOT_CHECK_HIP(hipMemset(h->q, 0, qkv * sizeof(bf16)));
  DFOT_CHECK_HIP(hipMemset(h->k, 0, qkv * sizeof(bf16)));
  DFOT_CHECK_HIP(hipMemset(h->v, 0, qkv * sizeof(bf16)));
  if ((rc = h->alloc(&h->hid, rows * c.mlp_hidden, true))) return rc;
  if ((rc = h->alloc(&h->idx, (size_t)max_batch * c.max_tokens, true))) return rc;
  h->max_batch = max_batch;
  return DFOT_OK;
}

size_t dfot_dit1d_workspace_bytes(dfot_dit1d_t h) { return h ? h->ws_bytes : 0; }

int dfot_dit1d_forward(dfot_dit1d_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens, void* stream) {
  DFOT_REQUIRE(h && x && noise_levels && out, DFOT_ERR_ARG, "dit1d forward: null argument");
  DFOT_REQUIRE(h->finalized, DFOT_ERR_STATE, "dit1d forward: weights not finalized");
  const dfot_dit1d_config& c = h->cfg;
  // the pos_embed add fixes the sequence length (dit_model.py:512): the reference runs at max_tokens only
  DFOT_REQUIRE(tokens == c.max_tokens, DFOT_ERR_SHAPE, "dit1d forward: %d tokens, the model runs at max_tokens = %d only", tokens, c.max_tokens);
  DFOT_REQUIRE(batch > 0 && batch <= h->max_batch, DFOT_ERR_STATE, "dit1d forward: batch %d exceeds the reserved %d", batch, h->max_batch);
  hipStream_t s = (hipStream_t)stream;
  const int hd = c.hidden, L = c.tokens_per_frame, n = h->ntok, frames = batch * tokens;
  const long rows = (long)batch * n;
  int rc = 0;
  if ((rc = launch_d1_clamp_levels(noise_levels, h->idx, frames, c.timesteps - 1, s))) return rc;
  if ((rc = launch_d1_tok_embed(x, h->x_w, h->x_b, h->pos, h->X, c.in_channels, L, n, hd, rows, s))) return rc;
  const float qscale = 1.4426950408889634f / sqrtf((float)h->d);  // attention works in the exp2 domain
  auto ln_share = [&](long off) -> int {
    return launch_d1_ln_share(h->X, h->A, h->mod_table, h->idx, h->ldt, off, hd, L, (int)rows, c.eps, s);
  };
  auto gated = [&](const bf16* a, int kdim, const bf16* w, const float* bias, long gate_off) -> int {
    GemmArgs g;  // X <- X + gate * (a W^T + bias), in place onto the normalised row
    g.A = a; g.lda = kdim; g.W = w; g.M = (int)rows; g.N = hd; g.K = kdim; g.bias = bias;
    g.out_f32 = h->X; g.ldo = hd; g.resid = h->X;
    g.gate = h->mod_table + gate_off; g.gate_index = h->idx; g.ldg = h->ldt; g.gate_rows = L;
    return launch_gemm(A_DENSE, E_F32, GEMM_AUTO, g, s);
  };
  for (const D1Block& w : h->blocks) {
    if ((rc = ln_share(w.mod))) return rc;
    {
      GemmArgs g;
      g.A = h->A; g.lda = hd; g.W = w.w_qkv; g.M = (int)rows; g.N = 3 * hd; g.K = hd; g.bias = w.b_qkv;
      g.q = h->q; g.k = h->k; g.v = h->v; g.rope_cs = nullptr; g.heads = c.heads; g.d = h->d;
      g.dstride = h->dstride; g.ntok = n; g.qscale = qscale;
      if ((rc = launch_gemm(A_DENSE, E_QKV_DIT, GEMM_AUTO, g, s))) return rc;
    }
    if (c.causal)
      rc = launch_attention_frame_causal(h->q, h->k, h->v, h->A, hd, batch, c.heads, n, L, h->d, s);
    else
      rc = launch_attention_padded(h->q, h->k, h->v, h->A, hd, batch, c.heads, n, h->d, s);
    if (rc) return rc;
    if ((rc = gated(h->A, hd, w.w_proj, w.b_proj, w.mod + 2 * hd))) return rc;
    if ((rc = ln_share(w.mod + 3 * hd))) return rc;
    {
      GemmArgs g;
      g.A = h->A; g.lda = hd; g.W = w.w_fc1; g.M = (int)rows; g.N = c.mlp_hidden; g.K = hd; g.bias = w.b_fc1;
      g.out_bf16 = h->hid; g.ldo = c.mlp_hidden; g.act = 1;
      if ((rc = launch_gemm(A_DENSE, E_BF16, GEMM_AUTO, g, s))) return rc;
    }
    if ((rc = gated(h->hid, c.mlp_hidden, w.w_fc2, w.b_fc2, w.mod + 5 * hd))) return rc;
  }
  return launch_d1_final(h->X, h->fin_w, h->fin_b, out, hd, c.in_channels, L, (int)rows, c.eps, s);
}

// ---- single launches of the forward (test entries: the engine's own launchers on caller-provided buffers) ----
static int op_d1_hidden(const char* what, int hidden) {
  DFOT_REQUIRE(hidden > 0 && hidden % 64 == 0 && hidden <= 2048, DFOT_ERR_SHAPE, "%s: hidden %d must be a multiple of 64, <= 2048", what, hidden);
  return DFOT_OK;
}

int dfot_op_dit1d_tok_embed(const float* x, const float* w, const float* b, const float* pos, float* X, int C, int L, int n, int hidden, int64_t rows,
                            void* stream) {
  DFOT_REQUIRE(x && w && b && pos && X, DFOT_ERR_ARG, "dit1d tok_embed: null argument");
  if (int rc = op_d1_hidden("dit1d tok_embed", hidden)) return rc;
  DFOT_REQUIRE(C > 0 && C <= 64, DFOT_ERR_SHAPE, "dit1d tok_embed: in_channels %d must be in [1, 64]", C);
  DFOT_REQUIRE(L > 0 && n > 0 && n % L == 0 && rows > 0 && rows % n == 0 && rows * (long)hidden < (1L << 31), DFOT_ERR_SHAPE,
               "dit1d tok_embed: %ld rows in sequences of %d tokens, %d per frame", (long)rows, n, L);
  return launch_d1_tok_embed(x, w, b, pos, X, C, L, n, hidden, (long)rows, (hipStream_t)stream);
}

int dfot_op_dit1d_ln_share(float* X, void* A, const float* table, const int32_t* levels, int32_t* idx, int64_t ldt, int64_t off, int hidden,
                           int rows_per_frame, int rows, float eps, int max_level, void* stream) {
  DFOT_REQUIRE(X && A && table && levels && idx, DFOT_ERR_ARG, "dit1d ln_share: null argument");
  if (int rc = op_d1_hidden("dit1d ln_share", hidden)) return rc;
  DFOT_REQUIRE(rows > 0 && rows_per_frame > 0 && rows % rows_per_frame == 0, DFOT_ERR_SHAPE, "dit1d ln_share: %d rows of %d per frame", rows,
               rows_per_frame);
  DFOT_REQUIRE(max_level >= 0 && off >= 0 && off % 4 == 0 && ldt % 4 == 0 && ldt >= off + 2L * hidden, DFOT_ERR_ARG,
               "dit1d ln_share: table row of %ld with (shift | scale) at %ld (multiples of 4), max_level %d", (long)ldt, (long)off, max_level);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_d1_clamp_levels(levels, idx, rows / rows_per_frame, max_level, s)) return rc;
  return launch_d1_ln_share(X, (bf16*)A, table, idx, ldt, off, hidden, rows_per_frame, rows, eps, s);
}

int dfot_op_dit1d_final(const float* X, const float* w, const float* b, float* out, int hidden, int C, int L, int rows, float eps, void* stream) {
  DFOT_REQUIRE(X && w && b && out, DFOT_ERR_ARG, "dit1d final: null argument");
  if (int rc = op_d1_hidden("dit1d final", hidden)) return rc;
  DFOT_REQUIRE(C > 0 && C <= 64 && L > 0 && rows > 0 && rows % L == 0, DFOT_ERR_SHAPE, "dit1d final: %d rows of %d per frame, %d channels", rows, L, C);
  return launch_d1_final(X, w, b, out, hidden, C, L, rows, eps, (hipStream_t)stream);
}

}  // extern "C"
