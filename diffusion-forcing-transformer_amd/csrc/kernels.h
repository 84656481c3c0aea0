// HBM-bound kernels of the DFoT backbone and sampler step (launch wrappers).
#pragma once
#include "common.h"

namespace dfot {

// ---- embeddings ----
int launch_noise_emb(const float* k, const float* freqs, const float* phases, const float* w1, const float* b1,
                     const float* w2, const float* b2, float* hidden, float* out, int bt, int ndim, int e, hipStream_t s);
// the pose-free UViT3D's per-frame embedding in one launch: Fourier noise-level MLP + (cond != nullptr, video not masked) action MLP
int launch_uvit3d_emb(const float* k, const float* freqs, const float* phases, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* cond, const uint8_t* cond_mask, const float* a_w1, const float* a_b1,
                      const float* a_w2, const float* a_b2, float* out, int bt, int ndim, int cdim, int e, int tokens, hipStream_t s);
int launch_embed_input(const float* x, const float* w, const float* b, float* out, int bt, int res, int cin, int c0,
                       hipStream_t s);
int launch_cond_repack(const float* cond, bf16* a, int bt, int res, int cdim, int kpad, hipStream_t s);
int launch_emb_pyramid(const bf16* emb0, bf16* emb1, bf16* emb2, bf16* emb3, int bt, int r0, int e, hipStream_t s);
// live (optional, device uint8 [bt]): frames whose flag is 0 are SKIPPED by the kernels that take it -- nothing read, nothing written
// (project_output writes zeros) -- for frames whose output the caller discards (the sampler's context tokens), uvit.hip
int launch_project_output(const float* x0, const float* w, const float* b, float* out, int bt, int res, int c0, int cout,
                          hipStream_t s, const uint8_t* live = nullptr);
// ---- norms ----
// GroupNorm(32): partial[bt][nblk][32][2] = (sum, sumsq) per block of pixels (standalone kernels below, or the fused
// GEMM epilogue with nblk = pixels/64); launch_gn_finalize reduces them deterministically to stats[bt][32][2] = (mean, rstd)
int launch_gn_partial_f32(const float* x, float* partial, int bt, int pixels, int c, hipStream_t s);
int launch_gn_partial_bf16(const bf16* x, float* partial, int bt, int pixels, int c, hipStream_t s);
int launch_gn_finalize(const float* partial, float* stats, int bt, int nblk, int pixels, int c, float eps, hipStream_t s);
int gn_partial_blocks(int pixels);
int launch_gn_apply_silu(const float* x, const float* stats, const float* gamma, const float* beta, bf16* out, int bt,
                         int pixels, int c, hipStream_t s, const uint8_t* live = nullptr);
// FiLM with the per-window pose cache (see kernels.hip). One FilmChunk per 64 rows of every FiLM projection:
struct FilmChunk {
  const bf16* w;   // &W_film[row0][0], row stride = emb dim
  const float* b;  // &bias[row0]
  long out_off;    // sv element (bt, r) of this chunk lives at out_off + bt*rows + r
  int rows;        // 2C of the owning block
};
int launch_film_vec(const FilmChunk* table, int chunks, const float* nemb, float* sv, int bt, int e, hipStream_t s);
// fcache == nullptr (here and in launch_rms_film*): the pose-free instantiation -- FiLM from sv alone, no fcache / cond_mask loads
int launch_gn_film_silu(const bf16* h, const float* stats, const float* gamma, const float* beta, const bf16* fcache,
                        const float* sv, const uint8_t* cond_mask, bf16* out, int bt, int pixels, int c, int tokens,
                        hipStream_t s, const uint8_t* live = nullptr);
// a residual stream whose last out-projection is still two or three K-slice partials: x += bias[c] + s0 + s1 (+ s2) (run_tr_block, uvit.hip)
struct RmsPending {
  void* x;  // where the completed sum goes: fp32 (launch_rms_film) or bf16 (launch_rms_film_bf16), the type of the stream
  const float* bias;
  const float* s0;
  const float* s1;
  const float* s2;  // optional third slice
};
int launch_rms_film(const float* x, const float* w, const bf16* fcache, const float* sv, const uint8_t* cond_mask, bf16* out,
                    long m, int c, int rows_per_bt, int tokens, float eps, hipStream_t s, const RmsPending* pend = nullptr);
int launch_rms_film_bf16(const bf16* x, const float* w, const bf16* fcache, const float* sv, const uint8_t* cond_mask, bf16* out,
                         long m, int c, int rows_per_bt, int tokens, float eps, hipStream_t s, const RmsPending* pend = nullptr);

// ---- resampling / skips ----
int launch_pool2_bf16(const float* x, bf16* out, int bt, int h, int w, int c, hipStream_t s);
// the same kernels on a bf16 residual stream (the inference engine's ResBlock levels)
int launch_pool2_bf16_bf16in(const bf16* x, bf16* out, int bt, int h, int w, int c, hipStream_t s);
int launch_sub_bf16_bf16in(const bf16* a, const float* b, bf16* out, long n, hipStream_t s, const uint8_t* live = nullptr, long frame_elems = 0);
int launch_upsample_add_bf16(const float* t, const bf16* skip, bf16* out, int bt, int h, int w, int c, hipStream_t s, const uint8_t* live = nullptr);
int launch_gn_apply_silu_bf16in(const bf16* x, const float* stats, const float* gamma, const float* beta, bf16* out, int bt, int pixels, int c,
                                hipStream_t s, const uint8_t* live = nullptr);
int launch_embed_input_bf16(const float* x, const float* w, const float* b, bf16* out, int bt, int res, int cin, int c0, hipStream_t s);
int launch_project_output_bf16(const bf16* x0, const float* w, const float* b, float* out, int bt, int res, int c0, int cout, hipStream_t s,
                               const uint8_t* live = nullptr);
int launch_sub_bf16(const float* a, const float* b, bf16* out, long n, hipStream_t s, const uint8_t* live = nullptr, long frame_elems = 0);
int launch_upsample_add(const float* t, const float* skip, float* out, int bt, int h, int w, int c, hipStream_t s, const uint8_t* live = nullptr);
// ---- pose ----
int launch_ray_encode(const float* poses, float* out, int b, int t, int res, int normalized, hipStream_t s);
// ---- sampler ----
int launch_hg_prepare(const float* x, const float* noise, const float* qa, const float* qb, float* x_in, int batch,
                      int nfe, int tokens, long f, hipStream_t s);
int launch_ddim_compose(const float* x, const float* x_in, const float* v, const float* sa, const float* s1,
                        const float* an, const float* cn, const float* keep, const float* weight, const uint8_t* gen,
                        float* x_next, int batch, int nfe, int tokens, long f, bool weight_per_token, hipStream_t s);
int launch_ddim_noise(const float* noise, const float* sigma, const float* weight, const uint8_t* gen, float* x_next, int batch, int nfe,
                      int tokens, long f, bool weight_per_token, hipStream_t s);
// v-prediction loss: partial = scratch [bt][vloss_chunks(f)], loss[bt] = mean over the frame of w*(eps_hat-eps)^2
int vloss_chunks(long f);
int launch_vloss(const float* x, const float* noise, const float* v, const float* a, const float* sg, const float* w,
                 float* x_pred, float* partial, float* loss, int batch, int tokens, long f, bool vspace, hipStream_t s);
// ---- weight-gradient GEMM over the token axis (wgrad.hip): out[slices][M][N] = partial sums of A^T B, A [rows][lda], B [rows][ldb] ----
int launch_wgrad_nt(const bf16* a, long lda, const bf16* b, long ldb, float* out, int m, int n, long rows, int slices, hipStream_t s, int img_h = 0,
                    int img_w = 0, int sdy = 0, int sdx = 0, int all_taps = 0);
// tile form (0: 128 x 128 / 4 waves; 1: 256 x 256 / 16; 2: 256 x 192 / 12; 3: 192 x 256 / 12) and K slices of one weight gradient
struct WgradPlan {
  int form, slices;
};
WgradPlan wgrad_plan(int m, int n, long rows, long max_slices);
int launch_wgrad_conv_taps(const bf16* dy, const bf16* x, float* out, int co, int ci, long pix, int slices, int img_h, int img_w, hipStream_t s);
int wgrad_conv_tiles(int co, int ci, int* target);
int launch_wgrad_nt_plan(const bf16* a, long lda, const bf16* b, long ldb, float* out, int m, int n, long rows, WgradPlan plan, hipStream_t s);
// ---- left-factor gradients of the FacMatDiT matrix block (facmat_factor_wgrad.hip): out[Ra][Rb] fp32 = sum_{f,d} A[f][ra][d] B[f][rb][d];
// A [frames][Ra][hd], B [frames][Rb][hd] bf16 read as they lie; Ra, Rb in {64, 128}, hd % 128 == 0, frames >= 1.  The frame axis is split
// over workgroups that store partial tiles to ws (ws_floats >= slices * Ra * Rb bounds the slice count; null: one slice, straight into
// out) and a second launch sums them in a fixed order: no atomics, the same bits every call
int launch_facmat_factor_wgrad(const bf16* a, const bf16* b, float* out, float* ws, size_t ws_floats, int frames, int ra, int rb, int hd,
                               hipStream_t s);
// the slice count of one call: a function of the shape and the device, at most max_slices (the workspace: slices * Ra * Rb floats)
int facmat_factor_wgrad_slices(int frames, int ra, int rb, long max_slices);
// ---- training: loss gradient, gradient norm, AdamW (flat fp32 buffers) ----
int launch_vloss_grad(const float* x, const float* noise, const float* v, const float* a, const float* sg, const float* coef, float* dv,
                      int batch, int tokens, long f, bool vspace, hipStream_t s);
int launch_sumsq(const float* x, long n, float* out, hipStream_t s);
int launch_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float wd, int step,
                 const float* sumsq, float max_norm, float* ema, float ema_decay, hipStream_t s);
// ---- casts / weight packing ----
int launch_f32_to_bf16(const float* src, bf16* dst, long n, hipStream_t s);
int launch_bf16_to_f32(const bf16* src, float* dst, long n, hipStream_t s);
// *differs = 1 (device int, zeroed by the caller on the same stream) when the two buffers differ in any bit; bytes == 0 launches nothing
int launch_equal_bits(const void* a, const void* b, long bytes, int* differs, hipStream_t s);
// dst[r][col0 + k] (row stride ldd) = src[map ? map[r] : r][k] for k < K ; zero for K <= k < kpad
int launch_pack_rows(const float* src, bf16* dst, const int* map, int rows, int k, int kpad, long ldd, int col0,
                     hipStream_t s);
// conv weight [Co][Ci][3][3] fp32 -> [Co][(ky*3+kx)*Ci + ci] bf16
int launch_pack_conv3(const float* src, bf16* dst, int co, int ci, hipStream_t s);
int launch_gather_f32(const float* src, float* dst, const int* map, int n, hipStream_t s);
// activation layout helpers for taps: [BT][P][C] fp32 -> [BT][C][P] fp32
int launch_nhwc_to_nchw(const float* src, float* dst, int bt, int p, int c, hipStream_t s);
int launch_bf16_nhwc_to_nchw(const bf16* src, float* dst, int bt, int p, int c, hipStream_t s);

// ---- attention forward ----
// fp32 partial rows (O | m, l) of the key-split tail of the level-2 / level-3 attention kernels.  A backbone handle owns one, sized by
// attention_scratch_bytes() in its reserve(); nullptr = the process-wide op-level scratch (grow-only, never freed: attention_split.hip)
struct AttnScratch {
  float* p = nullptr;
  size_t bytes = 0;
};
int launch_attention(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, int d,
                     int variant, hipStream_t stream, AttnScratch* scratch = nullptr);
// attention_v3.hip: d = 64, 64 query rows per wave, balanced tail (key-split left-over tiles + merge); nomax = caller bounds |score|
int launch_attention_v3(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, bool nomax,
                        hipStream_t stream, AttnScratch* scratch = nullptr);
// attention_v5.hip: attention_v3's NOMAX kernel with the key loop software-pipelined at half-tile granularity inside each wave;
// attention_v5_applies: the shape fits and the caller's bound of |score| (exp2 domain) allows a kernel without a running max
bool attention_v5_applies(int n, int d, float score_bound);
int launch_attention_v5(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, hipStream_t stream,
                        AttnScratch* scratch = nullptr, float* lse = nullptr);  // lse: [B][heads][N] log2-domain log-sum-exp (training)
// attention_ks.hip: 128-element rows, 8 waves per workgroup with the key axis split inside the workgroup (launches of few query tiles)
bool attention_ks_applies(int batch, int heads, int n, int d);
size_t attention_ks_scratch_bytes(int batch, int heads, int n, int d);
int launch_attention_ks(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, hipStream_t stream,
                        AttnScratch* scratch = nullptr);
int attention_dstride(int d);
// lse (optional, training): [B][heads][N] fp32, log2-domain log-sum-exp of every query row
int launch_attention_padded(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, int d,
                            hipStream_t stream, float* lse = nullptr);
// attention_seq64.hip: launch_attention_padded's operands and output with n = 64 (sequences shorter than that launcher's 128-row tile):
// one workgroup per (sequence, head), single-pass softmax.  d % 8 == 0, d <= 128, ldo % 8 == 0
int launch_attention_seq64(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int nseq, int heads, int d, hipStream_t stream);
// attention_seq64_bwd.hip: backward of launch_attention_seq64, the 64 x 64 problem recomputed in one launch (no lse, no delta, no o);
// d_o compact as that launcher's o; dq / dk / dv in the layout of q / k / v under the contract of launch_attention_bwd below (dq: gradient
// of the UNSCALED q, dk carrying ln 2), live columns only.  The forward's shape rules
int launch_attention_seq64_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dq, bf16* dk, bf16* dv, int nseq,
                               int heads, int d, hipStream_t s);
// the same kernel storing straight into the packed layout launch_qkv_grad_pack (no rope table) would give: row seq*64 + r of
// dqkv [nseq*64][ldg], dq at column head*d, dk at heads*d + head*d, dv at 2*heads*d + head*d; the same bits.  ldg >= 3*heads*d, ldg % 8 == 0
int launch_attention_seq64_bwd_packed(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dqkv, long ldg, int nseq,
                                      int heads, int d, hipStream_t s);
// attention_frame_causal.hip: launch_attention_padded's operands and output under the block-lower-triangular mask of the DiT1D backbone:
// query i sees key j iff j / frame_len <= i / frame_len.  frame_len in {16, 32, 64, 128}, n % 128 == 0, d % 8 == 0, d <= 128, ldo % 8 == 0
// lse (optional, training): [B][heads][N] fp32, log2-domain log-sum-exp of every query row; null launches the inference instantiation
int launch_attention_frame_causal(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, int frame_len,
                                  int d, hipStream_t stream, float* lse = nullptr);
// attention_temporal.hip: q, k, v [batch*tokens][heads][patches][dstride]; every (video, head, patch position) attends over its `tokens`
// frames (1 .. 32); o [(video, frame, patch)][ldo] compact.  patches % 64 == 0, d % 4 == 0
int launch_attention_temporal(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int tokens, int patches, int heads,
                              int d, hipStream_t s);
// attention_temporal_bwd.hip: backward of launch_attention_temporal, the T x T problem recomputed (no lse, no delta); d_o compact
// [(video, frame, patch)][ldo]; dq / dk / dv in the layout of q / k / v under the contract of launch_attention_bwd below (dq: gradient of
// the UNSCALED q), live columns only.  The forward's shape rules (patches % 64 == 0) with d % 8 == 0
int launch_attention_temporal_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dq, bf16* dk, bf16* dv,
                                  int batch, int tokens, int patches, int heads, int d, hipStream_t s);
// attention_matrix.hip: MatrixAttention core of the FacMatDiT backbone; z [batch*L*E][3h] (q|k|v), o [batch*L*E][h], one problem per
// (video, col head, row head), 1 <= L <= 32, (h / rr) % 4 == 0; rope_cs: [>= L][h/rr/2][2] (cos, sin) per frame, nullptr = no rotation
int launch_matrix_attn_rope(const bf16* z, bf16* o, const float* rope_cs, int batch, int L, int E, int h, int cc, int rr, float scale,
                            hipStream_t s);
// attention_matrix_bwd.hip: backward of launch_matrix_attn_rope; d_o [batch*L*E][h], dz [batch*L*E][3h] (dq|dk|dv); same shape rules
int launch_matrix_attn_rope_bwd(const bf16* z, const bf16* d_o, const float* rope_cs, bf16* dz, int batch, int L, int E, int h, int cc, int rr,
                                float scale, hipStream_t s);
// facmat_narrow.hip: the left factors of the MatrixDiTBlock at 1 <= E <= 32, in the natural layouts (no transposes around them):
//   contract: w [frames][E][h] = u [E][P] x m [frames][P][h];   expand: s [frames][P][h] = u [P][E] x o [frames][E][h]
// bf16 operands and outputs, fp32 sums in a fixed order per frame.  P % 64 == 0, h % 64 == 0, h <= 2048, 16-byte aligned pointers
int launch_facmat_contract(const bf16* m, const bf16* u, bf16* w, int frames, int P, int h, int E, hipStream_t s);
int launch_facmat_expand(const bf16* o, const bf16* u, bf16* sp, int frames, int P, int h, int E, hipStream_t s);
// ---- attention maps (attention_map.hip): fp32 softmax probabilities recomputed from the forward's q / k; read-only on q / k ----
// launch_attention_map: q, k as launch_attention_padded takes them, n = tokens * patches, patches % 64 == 0, 1 <= tokens <= 32.
//   full: out [B][heads][n][n] (part unused);  frame: out [B][heads][tokens][tokens], part = attention_map_part_floats() floats of scratch
size_t attention_map_part_floats(int batch, int heads, int n, int tokens);
int launch_attention_map(const bf16* q, const bf16* k, float* out, float* part, bool full, int batch, int heads, int n, int tokens, int d,
                         hipStream_t s);
// q, k as launch_attention_temporal takes them (patches % 64 == 0 suffices); out [B][heads][tokens][tokens] = mean over the patches
size_t attention_temporal_map_part_floats(int batch, int heads, int tokens, int patches);
int launch_attention_temporal_map(const bf16* q, const bf16* k, float* out, float* part, int batch, int tokens, int patches, int heads, int d,
                                  hipStream_t s);
// z, rope_cs, scale as launch_matrix_attn_rope takes them; out [B][cc][rr][L][L]
int launch_matrix_attn_map(const bf16* z, const float* rope_cs, float* out, int batch, int L, int E, int h, int cc, int rr, float scale,
                           hipStream_t s);
// ---- attention forward: key split of the last round + scratch (attention_split.hip; shared by v3, v5 and ks) ----
struct AttnSplit {
  int tiles, full, rem, nsplit;
  int slots;  // resident workgroups of one round: wgs_per_cu x the device's CU count
};
AttnSplit attn_plan_split(int batch, int heads, int n, int qrows, int wgs_per_cu);
size_t attn_partial_bytes(const AttnSplit& sp, int qrows, int dcols);  // dcols: 64 or 128 columns of O
size_t attention_scratch_bytes(int batch, int heads, int n, int d);    // what launch_attention(variant 2 / 5 / 6 / 14) needs
int attn_partials(const AttnSplit& sp, int qrows, int dcols, float** po, float** pml, AttnScratch* scratch);
int attn_launch_merge(const AttnSplit& sp, int qrows, int dcols, const float* po, const float* pml, bf16* o, long ldo, int n, int heads,
                      hipStream_t stream, float* lse = nullptr);
// ---- attention backward (attention_bwd.hip) ----
// delta[b][head][n] = sum_c d_o * o over the head's columns; o / d_o compact [B*N][ldo] (head hd at column hd*d), d % 8 == 0
int launch_attention_bwd_delta(const bf16* o, const bf16* d_o, long ldo, float* delta, int batch, int heads, int n, int d, hipStream_t s);
// q (pre-scaled as in the forward) / k / v / dq / dk / dv: [B][heads][N][dstride]; d_o compact; dq is the gradient of the UNSCALED q
int launch_attention_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, const float* l2, const float* delta,
                         bf16* dq, bf16* dk, bf16* dv, int batch, int heads, int n, int d, hipStream_t s);
// launch_attention_bwd's shape rules, for an entry point that launches something else first (the forward, the delta kernel): checked up
// front, a refused call launches nothing
int attention_bwd_shape_check(int n, int d, long ldo);
// the backward of launch_attention_frame_causal under launch_attention_bwd's contract (l2 = that forward's lse, delta from
// launch_attention_bwd_delta, dq the gradient of the UNSCALED q, dk carrying ln 2): the frame-causal instantiations of the same kernels,
// which stream only the tiles on and below the block diagonal.  The forward's shape rules
int launch_attention_frame_causal_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, const float* l2,
                                      const float* delta, bf16* dq, bf16* dk, bf16* dv, int batch, int heads, int n, int frame_len, int d,
                                      hipStream_t s);

}  // namespace dfot
