// Training path of the DiT1D backbone (dit1d.hip: share_norm blocks, frame-causal attention, frozen pos_embed): forward with saved
// activations, hand-written backward, gradients in one flat fp32 buffer in the reference's parameter order.  Call for call the DiT3D
// trainer above (dit_train.inl), whose launchers it shares; included after it at the end of dit.hip (same translation unit).
//
// A block (dit1d/dit_model.py:248-271):
//     n1 = LN(x) ; m1 = n1 (1 + sc1) + sh1 ; qkv = m1 Wqkv^T + b ; o = attention(q, k, v) ; a = o Wp^T + bp ; x_mid = n1 + g1 a
//     n2 = LN(x_mid) ; m2 = n2 (1 + sc2) + sh2 ; u = m2 W1^T + b1 ; y = GELU(u) W2^T + b2 ; x_out = n2 + g2 y
// Backward for dY = d x_out:  da = dY g2, dg2 = sum_rows dY y ; dh = da W2, dW2 = da^T h ; du = dh GELU'(u) ; dm2 = du W1, dW1 = du^T m2 ;
//     d x_mid = LN_share_bwd(dres = dY, dm = dm2) ; the attention half the same way with dres = d x_mid and dm = dqkv Wqkv.
// The residual base is the unmodulated n, so dY reaches n directly and only dm passes (1 + scale) and feeds dshift / dscale
// (dit1d_train.hip); the DiT3D blocks above add onto the modulated row and fold both into one gradient.
// The six modulations of a block are evaluated per frame from the live weights (the inference engine's per-level table is only valid for
// frozen weights).  pos_embed is a frozen parameter of the reference: a buffer here, outside the flat parameter / gradient buffers.
#include "dit1d_train.h"

namespace dfot {
namespace {

constexpr int D1T_FREQ = 256;  // TimestepEmbedder.frequency_embedding_size

struct D1TrainBlock {
  long o_qkv_w = 0, o_qkv_b = 0, o_proj_w = 0, o_proj_b = 0, o_fc1_w = 0, o_fc1_b = 0, o_fc2_w = 0, o_fc2_b = 0, o_mod_w = 0, o_mod_b = 0;
  long mod = 0;  // column of (shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp) in a table row
  bf16 *w_qkv = nullptr, *w_qkvT = nullptr, *w_proj = nullptr, *w_projT = nullptr, *w_fc1 = nullptr, *w_fc1T = nullptr, *w_fc2 = nullptr,
       *w_fc2T = nullptr;  // bf16 compute copies: [out][in] and [in][out]
  // saved activations
  float *N1 = nullptr, *rstd1 = nullptr, *lse = nullptr, *N2 = nullptr, *rstd2 = nullptr;
  bf16 *m1 = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *o = nullptr, *a = nullptr, *m2 = nullptr, *u = nullptr, *hact = nullptr,
       *y = nullptr;
};

struct D1Param {
  std::string name;
  std::vector<int64_t> shape;
  long offset = 0;
};

}  // namespace
}  // namespace dfot

struct dfot_dit1d_train_s {
  dfot_dit1d_config cfg{};
  int d = 0, dstride = 0, ntok = 0;  // head dim, q/k/v row stride, T * L
  long ldt = 0, total = 0;           // table row: depth * 6 * hidden; floats of the flat buffers
  std::vector<dfot::D1Param> params;
  std::vector<dfot::D1TrainBlock> blocks;
  float *params_f32 = nullptr, *grads = nullptr;  // attached flat buffers (owned by the caller)
  long o_x_w = 0, o_x_b = 0, o_t_w1 = 0, o_t_b1 = 0, o_t_w2 = 0, o_t_b2 = 0, o_fin_w = 0, o_fin_b = 0;
  std::vector<void*> owned, ws_owned;
  size_t ws_bytes = 0;
  float* pos = nullptr;  // pos_embed [ntok][hidden]: a buffer, never part of the flat buffers
  bool pos_loaded = false, synced = false;
  dfot::bf16 *w_mod = nullptr, *w_modT = nullptr;
  float *b_mod = nullptr, *freqs = nullptr;
  // workspace
  int max_batch = 0, fp = 0, batch = 0;
  const float* x_saved = nullptr;  // the forward's input (caller keeps it alive until backward)
  const float* d_embed = nullptr;  // after a backward: gradient w.r.t. the token embedding's output
  float *feat = nullptr, *h1 = nullptr, *a1 = nullptr, *cemb = nullptr, *mod_table = nullptr, *X = nullptr, *x_fin = nullptr;
  dfot::bf16 *semb = nullptr, *sembT = nullptr;
  float *dY = nullptr, *dM = nullptr, *stats = nullptr, *delta = nullptr, *dmod = nullptr, *dbmod = nullptr, *dsemb = nullptr, *dc = nullptr,
        *da1 = nullptr, *dh1 = nullptr, *dmod_part = nullptr, *dbias_part = nullptr, *wg_ws = nullptr, *sum_part = nullptr;
  size_t wg_ws_floats = 0;
  dfot::bf16 *da = nullptr, *dO = nullptr, *dq = nullptr, *dk = nullptr, *dv = nullptr, *dqkv = nullptr, *dh = nullptr, *T1 = nullptr, *T2 = nullptr,
             *dmod_bf = nullptr, *dmodT = nullptr;
};

namespace dfot {
namespace {

template <typename T>
int d1t_alloc(dfot_dit1d_train_s* h, T** out, size_t count, bool workspace = false) {
  void* p = nullptr;
  DFOT_CHECK_HIP(hipMalloc(&p, count * sizeof(T)));
  DFOT_CHECK_HIP(hipMemset(p, 0, count * sizeof(T)));
  (workspace ? h->ws_owned : h->owned).push_back(p);
  if (workspace) h->ws_bytes += count * sizeof(T);
  *out = (T*)p;
  return DFOT_OK;
}

}  // namespace
}  // namespace dfot

extern "C" {

int dfot_dit1d_train_destroy(dfot_dit1d_train_t h) {
  if (!h) return DFOT_OK;
  for (void* p : h->owned) (void)hipFree(p);
  for (void* p : h->ws_owned) (void)hipFree(p);
  delete h;
  return DFOT_OK;
}

int dfot_dit1d_train_create(const dfot_dit1d_config* cfg, dfot_dit1d_train_t* out) {
  DFOT_REQUIRE(cfg && out, DFOT_ERR_ARG, "dfot_dit1d_train_create: null argument");
  const dfot_dit1d_config& c = *cfg;
  // the limits of dfot_dit1d_create; the weight-gradient GEMMs tile a feature axis by 128, which narrows hidden and mlp_hidden
  DFOT_REQUIRE(c.hidden > 0 && c.hidden % 128 == 0 && c.hidden <= 2048, DFOT_ERR_SHAPE, "dit1d train: hidden %d must be a multiple of 128, <= 2048", c.hidden);
  DFOT_REQUIRE(c.heads > 0 && c.hidden % c.heads == 0, DFOT_ERR_SHAPE, "dit1d train: hidden %d not divisible by %d heads", c.hidden, c.heads);
  const int d = c.hidden / c.heads;
  DFOT_REQUIRE(d % 8 == 0 && d <= 128, DFOT_ERR_SHAPE, "dit1d train: head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(c.mlp_hidden > 0 && c.mlp_hidden % 128 == 0, DFOT_ERR_SHAPE, "dit1d train: mlp_hidden %d must be a positive multiple of 128", c.mlp_hidden);
  DFOT_REQUIRE(c.in_channels > 0 && c.in_channels <= 64, DFOT_ERR_SHAPE, "dit1d train: in_channels %d must be in [1, 64]", c.in_channels);
  const int L = c.tokens_per_frame;
  DFOT_REQUIRE(L == 16 || L == 32 || L == 64 || L == 128, DFOT_ERR_SHAPE, "dit1d train: tokens_per_frame %d not in {16, 32, 64, 128}", L);
  DFOT_REQUIRE(c.max_tokens > 0 && ((long)c.max_tokens * L) % 128 == 0 && (long)c.max_tokens * L <= (1 << 20), DFOT_ERR_SHAPE,
               "dit1d train: max_tokens %d x tokens_per_frame %d must be a multiple of 128", c.max_tokens, L);
  DFOT_REQUIRE(c.depth > 0 && c.timesteps > 0, DFOT_ERR_SHAPE, "dit1d train: bad depth %d / timesteps %d", c.depth, c.timesteps);
  DFOT_REQUIRE(c.causal == 0 || c.causal == 1, DFOT_ERR_ARG, "dit1d train: causal %d must be 0 or 1", c.causal);
  DFOT_REQUIRE(c.eps > 0.f, DFOT_ERR_ARG, "dit1d train: eps must be positive");
  auto* h = new dfot_dit1d_train_s();
  h->cfg = c;
  const int hd = c.hidden, mh = c.mlp_hidden;
  h->d = d;
  h->dstride = attention_dstride(d);
  h->ntok = c.max_tokens * L;
  h->ldt = (long)c.depth * 6 * hd;
  h->blocks.resize(c.depth);
  // the reference module's parameters() order (its state_dict order without the frozen pos_embed); every tensor 16-byte aligned
  auto add = [&](const std::string& name, std::vector<int64_t> shape) -> long {
    D1Param p;
    p.name = name;
    p.shape = shape;
    p.offset = h->total;
    long n = 1;
    for (int64_t v : shape) n *= v;
    h->total += (n + 3) / 4 * 4;
    h->params.push_back(p);
    return p.offset;
  };
  h->o_x_w = add("x_embedder.weight", {hd, c.in_channels});
  h->o_x_b = add("x_embedder.bias", {hd});
  h->o_t_w1 = add("t_embedder.mlp.0.weight", {hd, D1T_FREQ});
  h->o_t_b1 = add("t_embedder.mlp.0.bias", {hd});
  h->o_t_w2 = add("t_embedder.mlp.2.weight", {hd, hd});
  h->o_t_b2 = add("t_embedder.mlp.2.bias", {hd});
  for (int i = 0; i < c.depth; ++i) {
    D1TrainBlock& b = h->blocks[i];
    const std::string p = "blocks." + std::to_string(i) + ".";
    b.mod = (long)i * 6 * hd;
    b.o_qkv_w = add(p + "attn.qkv.weight", {3 * hd, hd});
    b.o_qkv_b = add(p + "attn.qkv.bias", {3 * hd});
    b.o_proj_w = add(p + "attn.proj.weight", {hd, hd});
    b.o_proj_b = add(p + "attn.proj.bias", {hd});
    b.o_fc1_w = add(p + "mlp.fc1.weight", {mh, hd});
    b.o_fc1_b = add(p + "mlp.fc1.bias", {mh});
    b.o_fc2_w = add(p + "mlp.fc2.weight", {hd, mh});
    b.o_fc2_b = add(p + "mlp.fc2.bias", {hd});
    b.o_mod_w = add(p + "adaLN_modulation.1.weight", {6 * hd, hd});
    b.o_mod_b = add(p + "adaLN_modulation.1.bias", {6 * hd});
  }
  h->o_fin_w = add("final_layer.1.weight", {c.in_channels, hd});
  h->o_fin_b = add("final_layer.1.bias", {c.in_channels});
  int rc = 0;
  auto fail = [&](int code) { dfot_dit1d_train_destroy(h); return code; };
  if ((rc = d1t_alloc(h, &h->w_mod, (size_t)h->ldt * hd)) || (rc = d1t_alloc(h, &h->w_modT, (size_t)h->ldt * hd)) ||
      (rc = d1t_alloc(h, &h->b_mod, (size_t)h->ldt)) || (rc = d1t_alloc(h, &h->pos, (size_t)h->ntok * hd)) ||
      (rc = d1t_alloc(h, &h->freqs, (size_t)D1T_FREQ / 2)))
    return fail(rc);
  std::vector<float> freqs(D1T_FREQ / 2);
  for (int i = 0; i < D1T_FREQ / 2; ++i)  // as dit1d.hip: torch.exp(-math.log(10000) * arange(half, dtype=float32) / half), fp32 throughout
    freqs[i] = expf((float)(-std::log(10000.0)) * (float)i / (float)(D1T_FREQ / 2));
  if (hipMemcpy(h->freqs, freqs.data(), freqs.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return fail(DFOT_ERR_HIP);
  for (D1TrainBlock& b : h->blocks)
    if ((rc = d1t_alloc(h, &b.w_qkv, (size_t)3 * hd * hd)) || (rc = d1t_alloc(h, &b.w_qkvT, (size_t)3 * hd * hd)) ||
        (rc = d1t_alloc(h, &b.w_proj, (size_t)hd * hd)) || (rc = d1t_alloc(h, &b.w_projT, (size_t)hd * hd)) ||
        (rc = d1t_alloc(h, &b.w_fc1, (size_t)mh * hd)) || (rc = d1t_alloc(h, &b.w_fc1T, (size_t)mh * hd)) ||
        (rc = d1t_alloc(h, &b.w_fc2, (size_t)mh * hd)) || (rc = d1t_alloc(h, &b.w_fc2T, (size_t)mh * hd)))
      return fail(rc);
  *out = h;
  return DFOT_OK;
}

int dfot_dit1d_train_num_params(dfot_dit1d_train_t h) { return h ? (int)h->params.size() : 0; }
const char* dfot_dit1d_train_param_name(dfot_dit1d_train_t h, int i) {
  return (h && i >= 0 && i < (int)h->params.size()) ? h->params[i].name.c_str() : nullptr;
}
int dfot_dit1d_train_param_shape(dfot_dit1d_train_t h, int i, int64_t shape[4], int* ndim) {
  DFOT_REQUIRE(h && i >= 0 && i < (int)h->params.size() && shape && ndim, DFOT_ERR_ARG, "dit1d train_param_shape: bad argument");
  *ndim = (int)h->params[i].shape.size();
  for (int j = 0; j < *ndim; ++j) shape[j] = h->params[i].shape[j];
  return DFOT_OK;
}
int64_t dfot_dit1d_train_param_offset(dfot_dit1d_train_t h, int i) {
  return (h && i >= 0 && i < (int)h->params.size()) ? h->params[i].offset : -1;
}
int64_t dfot_dit1d_train_total_numel(dfot_dit1d_train_t h) { return h ? h->total : 0; }

int dfot_dit1d_train_load_buffer(dfot_dit1d_train_t h, const char* name, const float* data, int64_t numel, void* stream) {
  DFOT_REQUIRE(h && name && data, DFOT_ERR_ARG, "dit1d train_load_buffer: null argument");
  DFOT_REQUIRE(!strcmp(name, "pos_embed"), DFOT_ERR_NAME, "dit1d train_load_buffer: unexpected key '%s' (the model's one buffer is pos_embed)", name);
  DFOT_REQUIRE(numel == (int64_t)h->ntok * h->cfg.hidden, DFOT_ERR_SHAPE, "dit1d train_load_buffer: size mismatch for 'pos_embed'");
  DFOT_CHECK_HIP(hipMemcpyAsync(h->pos, data, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  h->pos_loaded = true;
  return DFOT_OK;
}

int dfot_dit1d_train_attach(dfot_dit1d_train_t h, float* params, float* grads) {
  DFOT_REQUIRE(h && params && grads, DFOT_ERR_ARG, "dit1d train_attach: null argument");
  DFOT_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)grads & 15) == 0, DFOT_ERR_ARG, "dit1d train_attach: buffers must be 16-byte aligned");
  h->params_f32 = params;
  h->grads = grads;
  h->synced = false;
  return DFOT_OK;
}

// fp32 master weights -> bf16 compute copies ([out][in] and transposed), stacked modulation Linear; call after every optimizer step
int dfot_dit1d_train_sync_weights(dfot_dit1d_train_t h, void* stream) {
  DFOT_REQUIRE(h && h->params_f32, DFOT_ERR_STATE, "dit1d train_sync_weights: no parameter buffer attached");
  hipStream_t s = (hipStream_t)stream;
  const int hd = h->cfg.hidden, mh = h->cfg.mlp_hidden;
  const float* p = h->params_f32;
  int rc = 0;
  auto pair = [&](long o_w, bf16* as_stored, bf16* transposed, int R, int C) -> int {
    int r = launch_f32_to_bf16(p + o_w, as_stored, (long)R * C, s);
    return r ? r : tr_transpose(as_stored, transposed, R, C, s);
  };
  for (D1TrainBlock& b : h->blocks) {
    if ((rc = launch_f32_to_bf16(p + b.o_mod_w, h->w_mod + b.mod * hd, (long)6 * hd * hd, s))) return rc;
    DFOT_CHECK_HIP(hipMemcpyAsync(h->b_mod + b.mod, p + b.o_mod_b, (size_t)6 * hd * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = pair(b.o_qkv_w, b.w_qkv, b.w_qkvT, 3 * hd, hd)) || (rc = pair(b.o_proj_w, b.w_proj, b.w_projT, hd, hd)) ||
        (rc = pair(b.o_fc1_w, b.w_fc1, b.w_fc1T, mh, hd)) || (rc = pair(b.o_fc2_w, b.w_fc2, b.w_fc2T, hd, mh)))
      return rc;
  }
  if ((rc = tr_transpose(h->w_mod, h->w_modT, (int)h->ldt, hd, s))) return rc;
  h->synced = true;
  return DFOT_OK;
}

int dfot_dit1d_train_reserve(dfot_dit1d_train_t h, int max_batch) {
  DFOT_REQUIRE(h && max_batch > 0, DFOT_ERR_ARG, "dit1d train_reserve: bad argument");
  if (max_batch <= h->max_batch) return DFOT_OK;
  DFOT_CHECK_HIP(hipDeviceSynchronize());
  for (void* p : h->ws_owned) (void)hipFree(p);
  h->ws_owned.clear();
  h->ws_bytes = 0;
  h->max_batch = 0;
  const dfot_dit1d_config& c = h->cfg;
  const int hd = c.hidden, mh = c.mlp_hidden;
  const size_t rows = (size_t)max_batch * h->ntok;
  const int frames = max_batch * c.max_tokens;
  const int fp = (frames + 255) / 256 * 256;
  const size_t bhn = (size_t)max_batch * c.heads * h->ntok;
  const size_t qsz = bhn * h->dstride;
  const int widest = mh > 3 * hd ? mh : 3 * hd;
  int rc = 0;
#define WS(ptr, count) if ((rc = d1t_alloc(h, &(ptr), (count), true))) return rc
  WS(h->feat, (size_t)frames * D1T_FREQ); WS(h->h1, (size_t)frames * hd); WS(h->a1, (size_t)frames * hd); WS(h->cemb, (size_t)frames * hd);
  WS(h->semb, (size_t)fp * hd); WS(h->sembT, (size_t)fp * hd); WS(h->mod_table, (size_t)fp * h->ldt);
  WS(h->X, rows * hd); WS(h->x_fin, rows * hd);
  for (D1TrainBlock& b : h->blocks) {
    WS(b.N1, rows * hd); WS(b.rstd1, rows); WS(b.m1, rows * hd); WS(b.q, qsz); WS(b.k, qsz); WS(b.v, qsz); WS(b.lse, bhn); WS(b.o, rows * hd);
    WS(b.a, rows * hd); WS(b.N2, rows * hd); WS(b.rstd2, rows); WS(b.m2, rows * hd); WS(b.u, rows * mh); WS(b.hact, rows * mh); WS(b.y, rows * hd);
  }
  h->wg_ws_floats = (size_t)3 * widest * hd;
  WS(h->wg_ws, h->wg_ws_floats);
  WS(h->dY, rows * hd); WS(h->dM, rows * hd); WS(h->stats, rows * 2); WS(h->delta, bhn);
  WS(h->dmod, (size_t)fp * h->ldt); WS(h->dmod_bf, (size_t)fp * h->ldt); WS(h->dmodT, (size_t)fp * h->ldt); WS(h->dbmod, (size_t)h->ldt);
  WS(h->dmod_part, (size_t)TR_CHUNKS * frames * h->ldt); WS(h->dbias_part, (size_t)TR_CHUNKS * frames * hd);
  WS(h->dsemb, (size_t)fp * hd); WS(h->dc, (size_t)frames * hd); WS(h->da1, (size_t)frames * hd); WS(h->dh1, (size_t)frames * hd);
  WS(h->sum_part, d1_wgrad_part_floats((long)rows, c.in_channels, hd, hd));  // nb = hidden >= in_channels: covers both weight gradients
  WS(h->da, rows * hd); WS(h->dO, rows * hd); WS(h->dq, qsz); WS(h->dk, qsz); WS(h->dv, qsz);
  WS(h->dqkv, rows * 3 * hd); WS(h->dh, rows * mh); WS(h->T1, rows * widest); WS(h->T2, rows * widest);
#undef WS
  h->max_batch = max_batch;
  h->fp = fp;
  return DFOT_OK;
}

// out[B,T,C,1,L] = model(x, levels) with every activation the backward needs kept in the workspace; x must stay alive until backward
int dfot_dit1d_train_forward(dfot_dit1d_train_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens, void* stream) {
  DFOT_REQUIRE(h && x && noise_levels && out, DFOT_ERR_ARG, "dit1d train_forward: null argument");
  DFOT_REQUIRE(h->pos_loaded, DFOT_ERR_STATE, "dit1d train_forward: load pos_embed with dfot_dit1d_train_load_buffer first");
  DFOT_REQUIRE(h->synced, DFOT_ERR_STATE, "dit1d train_forward: call dfot_dit1d_train_sync_weights after attaching / updating the parameters");
  const dfot_dit1d_config& c = h->cfg;
  DFOT_REQUIRE(tokens == c.max_tokens, DFOT_ERR_SHAPE, "dit1d train_forward: %d tokens, the model runs at max_tokens = %d only", tokens, c.max_tokens);
  DFOT_REQUIRE(batch > 0 && batch <= h->max_batch, DFOT_ERR_STATE, "dit1d train_forward: batch %d exceeds the reserved %d", batch, h->max_batch);
  static_assert(D1_DMOD_PLANES == TR_CHUNKS, "dit1d_train.hip writes the dmod_part layout of this translation unit");
  hipStream_t s = (hipStream_t)stream;
  const int hd = c.hidden, mh = c.mlp_hidden, L = c.tokens_per_frame, n = h->ntok, frames = batch * tokens;
  const long rows = (long)batch * n;
  const float* p = h->params_f32;
  int rc = 0;
  h->batch = batch; h->x_saved = x; h->d_embed = nullptr;
  // ---- conditioning: t = Linear2(SiLU(Linear1([cos | sin](level)))) per frame; table = Linear_mod(SiLU(t)) ----
  hipLaunchKernelGGL(tr_features_kernel, dim3(cdiv((long)frames * D1T_FREQ, 256)), dim3(256), 0, s, h->freqs, noise_levels, h->feat, frames, D1T_FREQ,
                     c.timesteps - 1);
  hipLaunchKernelGGL(rows_linear_kernel<0>, dim3(cdiv(hd, 4), frames), dim3(256), 0, s, h->feat, p + h->o_t_w1, p + h->o_t_b1, h->h1, (bf16*)nullptr,
                     D1T_FREQ, hd);
  hipLaunchKernelGGL(silu_fwd_kernel, dim3(cdiv((long)frames * hd, 256)), dim3(256), 0, s, h->h1, h->a1, (long)frames * hd);
  DFOT_CHECK_HIP(hipMemsetAsync(h->semb, 0, (size_t)h->fp * hd * sizeof(bf16), s));
  hipLaunchKernelGGL(rows_linear_kernel<0>, dim3(cdiv(hd, 4), frames), dim3(256), 0, s, h->a1, p + h->o_t_w2, p + h->o_t_b2, h->cemb, h->semb, hd, hd);
  DFOT_CHECK_HIP(hipGetLastError());
  {
    GemmArgs g;
    g.A = h->semb; g.lda = hd; g.W = h->w_mod; g.M = h->fp; g.N = (int)h->ldt; g.K = hd; g.bias = h->b_mod; g.out_f32 = h->mod_table; g.ldo = h->ldt;
    if ((rc = launch_gemm(A_DENSE, E_F32, GEMM_AUTO, g, s))) return rc;
  }
  if ((rc = d1_tok_embed(x, p + h->o_x_w, p + h->o_x_b, h->pos, h->X, c.in_channels, L, n, hd, rows, s))) return rc;
  const float qscale = 1.4426950408889634f / sqrtf((float)h->d);
  for (size_t bi = 0; bi < h->blocks.size(); ++bi) {
    D1TrainBlock& b = h->blocks[bi];
    float* next = bi + 1 < h->blocks.size() ? h->X : h->x_fin;
    if ((rc = launch_d1_ln_share_train(h->X, b.N1, b.rstd1, b.m1, h->mod_table, h->ldt, b.mod, hd, L, (int)rows, c.eps, s))) return rc;
    {
      GemmArgs g;
      g.A = b.m1; g.lda = hd; g.W = b.w_qkv; g.M = (int)rows; g.N = 3 * hd; g.K = hd; g.bias = p + b.o_qkv_b;
      g.q = b.q; g.k = b.k; g.v = b.v; g.rope_cs = nullptr; g.heads = c.heads; g.d = h->d; g.dstride = h->dstride; g.ntok = n; g.qscale = qscale;
      if ((rc = launch_gemm(A_DENSE, E_QKV_DIT, GEMM_AUTO, g, s))) return rc;
    }
    if (c.causal)
      rc = launch_attention_frame_causal(b.q, b.k, b.v, b.o, hd, batch, c.heads, n, L, h->d, s, b.lse);
    else
      rc = launch_attention_padded(b.q, b.k, b.v, b.o, hd, batch, c.heads, n, h->d, s, b.lse);
    if (rc) return rc;
    if ((rc = tr_gemm_bf16(b.o, hd, b.w_proj, (int)rows, hd, hd, p + b.o_proj_b, b.a, hd, s))) return rc;
    if ((rc = launch_gate_combine(b.N1, h->X, b.a, h->mod_table, h->ldt, b.mod + 2 * hd, hd, L, rows, s))) return rc;  // x_mid
    if ((rc = launch_d1_ln_share_train(h->X, b.N2, b.rstd2, b.m2, h->mod_table, h->ldt, b.mod + 3 * hd, hd, L, (int)rows, c.eps, s))) return rc;
    {
      GemmArgs g;  // h = GELU(u), u = m2 W1^T + b1: both kept (u for GELU', h for the fc2 weight gradient)
      g.A = b.m2; g.lda = hd; g.W = b.w_fc1; g.M = (int)rows; g.N = mh; g.K = hd; g.bias = p + b.o_fc1_b; g.out_bf16 = b.hact; g.ldo = mh;
      g.act = 1; g.pre_act = b.u;
      if ((rc = launch_gemm(A_DENSE, E_BF16, GEMM_AUTO, g, s))) return rc;
    }
    if ((rc = tr_gemm_bf16(b.hact, mh, b.w_fc2, (int)rows, hd, mh, p + b.o_fc2_b, b.y, hd, s))) return rc;
    if ((rc = launch_gate_combine(b.N2, next, b.y, h->mod_table, h->ldt, b.mod + 5 * hd, hd, L, rows, s))) return rc;
  }
  return d1_final(h->x_fin, p + h->o_fin_w, p + h->o_fin_b, out, hd, c.in_channels, L, (int)rows, c.eps, s);
}

// gradients of every parameter for the upstream gradient d_out [B,T,C,1,L] of the last forward's output; OVERWRITES the grads buffer
int dfot_dit1d_train_backward(dfot_dit1d_train_t h, const float* d_out, void* stream) {
  DFOT_REQUIRE(h && d_out, DFOT_ERR_ARG, "dit1d train_backward: null argument");
  DFOT_REQUIRE(h->batch > 0 && h->x_saved, DFOT_ERR_STATE, "dit1d train_backward: no forward to differentiate");
  const dfot_dit1d_config& c = h->cfg;
  const int batch = h->batch, hd = c.hidden, mh = c.mlp_hidden, L = c.tokens_per_frame, n = h->ntok, frames = batch * c.max_tokens, fp = h->fp;
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)batch * n;
  const float* p = h->params_f32;
  float* G = h->grads;
  float *dY = h->dY, *dM = h->dM;
  int rc = 0;
  if ((rc = zero_fill(G, (size_t)h->total * sizeof(float), s))) return rc;
  if ((rc = zero_fill(h->dmod, (size_t)fp * h->ldt * sizeof(float), s))) return rc;
  if ((rc = zero_fill(h->dmod_part, (size_t)TR_CHUNKS * frames * h->ldt * sizeof(float), s))) return rc;
  // dW[M][N] = dy^T x over the token rows: operands in place when the shape allows, else through transposed copies
  auto wgrad = [&](const bf16* dyp, int M, const bf16* xp, int N, float* outp) -> int {
    int r = tr_wgrad_nt(dyp, M, xp, N, M, N, rows, outp, s, h->wg_ws, h->wg_ws_floats);
    if (r != DFOT_ERR_STATE) return r;
    if ((r = tr_transpose(dyp, h->T1, (int)rows, M, s)) || (r = tr_transpose(xp, h->T2, (int)rows, N, s))) return r;
    return tr_wgrad(h->T1, h->T2, M, N, (int)rows, outp, s, h->wg_ws, h->wg_ws_floats);
  };
  auto gate_bwd = [&](const bf16* a, long gate_off, float* dbias) -> int {  // h->da = dY * gate, dgate into dmod_part, row sums of da into dbias
    return launch_gate_bwd(dY, a, h->mod_table, h->ldt, gate_off, h->da, h->dmod_part, h->dbias_part, dbias, hd, L, frames, s);
  };
  auto ln_bwd = [&](const float* N, const float* rstd, long off) -> int {  // dY <- d x for dres = dY and dm = dM
    return launch_d1_ln_share_bwd(dY, dM, N, rstd, h->mod_table, h->ldt, off, dY, h->dmod_part, hd, L, frames, s);
  };
  // ---- final layer: out = Linear(LN(x_fin)) ----
  if ((rc = launch_d1_final_dgrad(d_out, h->x_fin, p + h->o_fin_w, dY, h->stats, hd, c.in_channels, L, (int)rows, c.eps, s))) return rc;
  if ((rc = launch_d1_final_wgrad(d_out, h->x_fin, h->stats, h->sum_part, G + h->o_fin_w, G + h->o_fin_b, hd, c.in_channels, L, rows, s))) return rc;
  // ---- blocks, last to first ----
  for (int bi = (int)h->blocks.size() - 1; bi >= 0; --bi) {
    D1TrainBlock& b = h->blocks[bi];
    if ((rc = gate_bwd(b.y, b.mod + 5 * hd, G + b.o_fc2_b))) return rc;
    if ((rc = tr_gemm_bf16(h->da, hd, b.w_fc2T, (int)rows, mh, hd, nullptr, h->dh, mh, s))) return rc;  // dh = da W2
    if ((rc = wgrad(h->da, hd, b.hact, mh, G + b.o_fc2_w))) return rc;                                   // dW2 = da^T h
    if ((rc = launch_gelu(b.u, nullptr, h->dh, rows * mh, s))) return rc;                                // du
    if ((rc = launch_colsum_bf16(h->dh, G + b.o_fc1_b, rows, mh, (long)mh, s))) return rc;
    if ((rc = tr_gemm_f32(h->dh, mh, b.w_fc1T, (int)rows, hd, mh, dM, hd, nullptr, s))) return rc;       // dm2 = du W1 (NOT added to dY)
    if ((rc = wgrad(h->dh, mh, b.m2, hd, G + b.o_fc1_w))) return rc;                                     // dW1 = du^T m2
    if ((rc = ln_bwd(b.N2, b.rstd2, b.mod + 3 * hd))) return rc;                                         // dY = d x_mid
    if ((rc = gate_bwd(b.a, b.mod + 2 * hd, G + b.o_proj_b))) return rc;
    if ((rc = tr_gemm_bf16(h->da, hd, b.w_projT, (int)rows, hd, hd, nullptr, h->dO, hd, s))) return rc;  // dO = da Wp
    if ((rc = wgrad(h->da, hd, b.o, hd, G + b.o_proj_w))) return rc;                                     // dWp = da^T o
    if ((rc = launch_attention_bwd_delta(b.o, h->dO, hd, h->delta, batch, c.heads, n, h->d, s))) return rc;
    if (c.causal)
      rc = launch_attention_frame_causal_bwd(b.q, b.k, b.v, h->dO, hd, b.lse, h->delta, h->dq, h->dk, h->dv, batch, c.heads, n, L, h->d, s);
    else
      rc = launch_attention_bwd(b.q, b.k, b.v, h->dO, hd, b.lse, h->delta, h->dq, h->dk, h->dv, batch, c.heads, n, h->d, s);
    if (rc) return rc;
    if ((rc = launch_qkv_grad_pack(h->dq, h->dk, h->dv, nullptr, h->dqkv, rows, n, c.heads, h->d, h->dstride, s))) return rc;
    if ((rc = launch_colsum_bf16(h->dqkv, G + b.o_qkv_b, rows, 3 * hd, (long)3 * hd, s))) return rc;
    if ((rc = tr_gemm_f32(h->dqkv, 3 * hd, b.w_qkvT, (int)rows, hd, 3 * hd, dM, hd, nullptr, s))) return rc;  // dm1 = dqkv Wqkv
    if ((rc = wgrad(h->dqkv, 3 * hd, b.m1, hd, G + b.o_qkv_w))) return rc;                                    // dWqkv = dqkv^T m1
    if ((rc = ln_bwd(b.N1, b.rstd1, b.mod))) return rc;                                                       // dY = d x_in
  }
  // ---- token embedding (pos_embed is frozen: nothing for it) ----
  if ((rc = launch_d1_tok_embed_wgrad(dY, h->x_saved, h->sum_part, G + h->o_x_w, G + h->o_x_b, c.in_channels, L, hd, rows, s))) return rc;
  h->d_embed = dY;
  // ---- modulation Linears: table = SiLU(t) W_mod^T + b_mod over the frames (the tail of dfot_dit_train_backward) ----
  if ((rc = launch_dmod_reduce(h->dmod_part, h->dmod, (long)frames * h->ldt, s))) return rc;
  hipLaunchKernelGGL(frames_colsum_kernel, dim3(cdiv(h->ldt, 256)), dim3(256), 0, s, h->dmod, h->dbmod, frames, h->ldt);
  DFOT_CHECK_HIP(hipGetLastError());
  if ((rc = launch_f32_to_bf16(h->dmod, h->dmod_bf, (long)fp * h->ldt, s))) return rc;
  hipLaunchKernelGGL(pack_transpose_kernel, dim3(cdiv((long)fp * h->ldt, 256)), dim3(256), 0, s, h->dmod, h->dmodT, fp, (int)h->ldt);
  DFOT_CHECK_HIP(hipGetLastError());
  if ((rc = tr_transpose(h->semb, h->sembT, fp, hd, s))) return rc;
  for (D1TrainBlock& b : h->blocks) {  // dW_mod = dmod^T SiLU(t), written straight into the block's gradient tensor
    if ((rc = tr_gemm_f32(h->dmodT + b.mod * fp, fp, h->sembT, 6 * hd, hd, fp, G + b.o_mod_w, hd, nullptr, s))) return rc;
    DFOT_CHECK_HIP(hipMemcpyAsync(G + b.o_mod_b, h->dbmod + b.mod, (size_t)6 * hd * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  if ((rc = tr_wgrad(h->dmod_bf, h->w_modT, fp, hd, (int)h->ldt, h->dsemb, s, h->wg_ws, h->wg_ws_floats))) return rc;  // d SiLU(t) = dmod W_mod
  // ---- noise-level embedding MLP (frames x hidden, fp32) ----
  const long fh = (long)frames * hd;
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv(fh, 256)), dim3(256), 0, s, h->dsemb, h->cemb, h->dc, fh);
  hipLaunchKernelGGL(small_wgrad_kernel, dim3(cdiv((long)hd * hd, 256)), dim3(256), 0, s, h->dc, h->a1, G + h->o_t_w2, G + h->o_t_b2, frames, hd, hd);
  hipLaunchKernelGGL(small_dgrad_kernel, dim3(cdiv(fh, 256)), dim3(256), 0, s, h->dc, p + h->o_t_w2, h->da1, frames, hd, hd);
  hipLaunchKernelGGL(silu_bwd_kernel, dim3(cdiv(fh, 256)), dim3(256), 0, s, h->da1, h->h1, h->dh1, fh);
  hipLaunchKernelGGL(small_wgrad_kernel, dim3(cdiv((long)hd * D1T_FREQ, 256)), dim3(256), 0, s, h->dh1, h->feat, G + h->o_t_w1, G + h->o_t_b1, frames,
                     hd, D1T_FREQ);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// d(sum(out * d_out)) / d x for the last forward / backward pair: the data gradient of the token embedding (pos_embed and the
// noise-level path do not depend on x)
int dfot_dit1d_train_input_grad(dfot_dit1d_train_t h, float* dx, void* stream) {
  DFOT_REQUIRE(h && dx, DFOT_ERR_ARG, "dit1d train_input_grad: null argument");
  DFOT_REQUIRE(h->batch > 0 && h->d_embed, DFOT_ERR_STATE, "dit1d train_input_grad: run dfot_dit1d_train_backward first");
  const dfot_dit1d_config& c = h->cfg;
  return launch_d1_tok_embed_dgrad(h->d_embed, h->params_f32 + h->o_x_w, dx, c.in_channels, c.tokens_per_frame, c.hidden, (long)h->batch * h->ntok,
                                   (hipStream_t)stream);
}

}  // extern "C"
