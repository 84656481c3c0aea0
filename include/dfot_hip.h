/* dfot_hip.h -- C ABI of libdfot_hip.so: the MI355X (gfx950) DFoT denoising engine.
 *
 * Drop-in boundary for the reference's hot path (ktncktnc/diffusion-forcing-transformer):
 *   - dfot_uvit_*      replaces   UViT3DPose / BaseBackbone.forward
 *                                 algorithms/dfot/backbones/u_vit/u_vit3d_pose.py:63-131
 *                                 algorithms/dfot/backbones/base_backbone.py:78-86
 *                                 (called from diffusion/continuous_diffusion.py:119-121)
 *   - dfot_ray_encode  replaces   DFoTVideoPose._process_conditions (ray_encoding)
 *                                 algorithms/dfot/dfot_video_pose.py:64-110, utils/geometry_utils.py:49-81,244-295
 *   - dfot_hg_prepare  replaces   HistoryGuidance prepare (q_sample of history tokens per branch)
 *                                 algorithms/dfot/history_guidance.py:446-543,929-973 ; discrete_diffusion.py:242-250
 *   - dfot_ddim_compose replaces  v->x0/eps, ddim_sample_step, HG compose, context clamp
 *                                 diffusion/discrete_diffusion.py:213-223,454-538 ; history_guidance.py:545-568,978-982 ;
 *                                 dfot_video.py:750-752
 *   - dfot_dit_*       replaces   DiT3D / BaseBackbone.forward (Kinetics-600 backbone: DiTBase "full" variant, rope_3d)
 *                                 algorithms/dfot/backbones/dit/dit3d.py:146-192, dit/dit_base.py:150-196,391-419,
 *                                 dit/dit_blocks.py:49-128,378-542 (called from diffusion/discrete_diffusion.py:173-174)
 *   - dfot_op_*        unit-testable primitives the backbone is built from (GEMM / conv / attention / norms)
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every data pointer is a DEVICE
 * pointer unless it says "host".  `stream` is a hipStream_t passed as void*.  All functions return
 * 0 (DFOT_OK) or a DFOT_ERR_* code; dfot_last_error() returns the message of the last failure on
 * the calling thread.  Nothing here allocates or synchronises inside forward/step calls (graph-capturable)
 * except dfot_uvit_reserve / dfot_uvit_create / dfot_uvit_load_weight.
 */
#ifndef DFOT_HIP_H_
#define DFOT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DFOT_OK = 0,
  DFOT_ERR_ARG = 1,    /* null pointer / bad enum                      (reference: TypeError/ValueError) */
  DFOT_ERR_SHAPE = 2,  /* shape or length violates the contract        (reference: ValueError / assert)   */
  DFOT_ERR_HIP = 3,    /* a HIP runtime call failed                                                      */
  DFOT_ERR_STATE = 4,  /* weights missing / workspace not reserved                                        */
  DFOT_ERR_NAME = 5    /* unknown state-dict key                       (reference: load_state_dict strict) */
};

typedef struct dfot_uvit_s* dfot_uvit_t;

/* Hyper-parameters of u_vit3d_pose (configurations/algorithm/backbone/u_vit3d_pose.yaml:1-14 overridden by
 * configurations/dataset_experiment/realestate10k_video_generation.yaml:39-44). block types are fixed to
 * [ResBlock, ResBlock, TransformerBlock, TransformerBlock] with RoPE-3D, as on every BASELINE config. */
typedef struct {
  int32_t channels[4];
  int32_t emb_channels;
  int32_t num_updown_blocks[3];
  int32_t num_mid_blocks;
  int32_t num_heads;
  int32_t in_channels;   /* 3 */
  int32_t resolution;    /* x_shape[-1], e.g. 256 */
  int32_t max_tokens;    /* temporal length T, 8 */
  int32_t cond_dim;      /* 180 (ray_encoding) */
  int32_t noise_dim;     /* 256 */
  float rope_theta;      /* 10000 */
  float eps;             /* 1e-6 */
} dfot_uvit_config;

const char* dfot_last_error(void);
int dfot_version(void);

/* ---- backbone handle ------------------------------------------------------------------------- */
int dfot_uvit_create(const dfot_uvit_config* cfg, dfot_uvit_t* out);
int dfot_uvit_destroy(dfot_uvit_t h);
/* state-dict inventory (reference key names) */
int dfot_uvit_num_params(dfot_uvit_t h);
const char* dfot_uvit_param_name(dfot_uvit_t h, int index);
int dfot_uvit_param_shape(dfot_uvit_t h, int index, int64_t shape[4], int* ndim);
/* copy one fp32 tensor (device pointer, contiguous, reference layout) into the engine's packed bf16/fp32 layout */
int dfot_uvit_load_weight(dfot_uvit_t h, const char* name, const float* data, const int64_t* shape, int ndim,
                          void* stream);
/* verify every key was loaded; build derived tables (RoPE cos/sin, fused out-projection bias) */
int dfot_uvit_finalize(dfot_uvit_t h, void* stream);
/* allocate activations for a model batch of up to `max_batch` videos (B*NFE) */
int dfot_uvit_reserve(dfot_uvit_t h, int max_batch);
size_t dfot_uvit_workspace_bytes(dfot_uvit_t h);
/* tuning/debug switches: "gemm_variant" (-1 auto, else a tile form as in dfot_op_gemm),
 * "attn_variant" (2 = tuned kernel (default), 0 = baseline with transposed LDS reads for V, 1 = baseline with scalar LDS reads,
 * 3 = tuned kernel with two K/V stages, 4 = two stages + per-tile Q reload (4 waves per SIMD; slower, kept for A/B)), "time_attn" (see below) */
int dfot_uvit_set_option(dfot_uvit_t h, const char* key, int value);
/* also: "attn_force_safe" (1 = level-2 attention always takes the running-max kernel, as weights with a large QK-norm bound would)
 * Read-outs (valid after finalize), by key: "score_bound_l2" = the largest bound of |q.k| log2(e)/sqrt(d) over the level-2 blocks, from
 * their q_norm / k_norm weights (u_vit_blocks.py:255-262); "attn_kernel_l2" = 14 (no running max, bound < 64) or 5 (running max):
 * the level-2 attention kernel forward runs; "cond_builds" = the number of dfot_uvit_set_conditions calls on this handle (those of
 * dfot_uvit_forward included) that passed their argument checks: what a caller's conditioning cache did NOT save */
int dfot_uvit_query(dfot_uvit_t h, const char* key, double* value);
/* "time_attn" = N > 0 records HIP events (on the launch stream) around the next N level-2 attention launches;
 * this call synchronises on them, returns the summed duration and the number of launches, and resets the count */
int dfot_uvit_attn_timing(dfot_uvit_t h, double* total_ms, int64_t* launches);

/* out[B,T,C,H,W] = model(x[B,T,C,H,W], noise_levels[B,T], external_cond[B,T,180,H,W], external_cond_mask[B])
 * all fp32 contiguous; noise_levels is the float level the reference passes (0.125*logsnr[k]);
 * external_cond_mask: NULL or B bytes, non-zero => that video's pose embedding is zeroed.
 * Inputs are not modified. */
int dfot_uvit_forward(dfot_uvit_t h, const float* x, const float* noise_levels, const float* external_cond,
                      const uint8_t* external_cond_mask, float* out, int batch, void* stream);
/* The camera-pose conditioning of a window does not change across its DDIM steps (and is zero for masked
 * videos), and every FiLM projection is linear in it.  dfot_uvit_set_conditions computes the pose patch-embedding,
 * its pyramid and every block's FiLM projection of it ONCE; dfot_uvit_forward_cached then runs the backbone for the
 * cached conditions (batch must match).  dfot_uvit_forward == set_conditions + forward_cached. */
int dfot_uvit_set_conditions(dfot_uvit_t h, const float* external_cond, const uint8_t* external_cond_mask, int batch,
                             void* stream);
int dfot_uvit_forward_cached(dfot_uvit_t h, const float* x, const float* noise_levels, float* out, int batch,
                             void* stream);
/* The same with a per-frame flag (device uint8 [batch * T], or NULL = every frame): the rows of `out` of frames whose flag is 0 are not
 * computed (zeros are written).  The sampler's composition step (history_guidance.py:545-568, dfot_video.py:750-752) never reads the
 * model output of context tokens; past the last transformer block the U-Net works frame by frame (ResBlocks, up-convolutions, output
 * projection: u_vit3d.py:30-185), so those frames are skipped there.  Attention levels always run on every frame (context frames are keys). */
int dfot_uvit_forward_cached_live(dfot_uvit_t h, const float* x, const float* noise_levels, float* out, int batch,
                                  const uint8_t* live_frames, void* stream);
/* ... and with a second flag per frame (device uint8 [batch * T], or NULL = every frame is fresh): fresh_frames == 0 states that this frame's
 * input, noise level and conditioning are those of the PREVIOUS forward of this handle (same batch) -- a clean context frame of the
 * conditional History-Guidance branch keeps its value and its level over the DDIM steps of a window (dfot_video.py:682-752) -- so its
 * activations in the frame-local down path (ResBlock levels, Downsample convolutions) are still in the workspace and are not recomputed.
 * A frozen frame must be a dead frame (live_frames == 0) in this forward AND in the previous one -- the up path overwrites the level
 * buffers of live frames in place -- so live_frames may not be NULL (DFOT_ERR_ARG).  DFOT_ERR_STATE when the previous forward ran another
 * batch.  The flags are ignored (everything is recomputed) when an image of the third level has fewer rows than the largest GEMM tile
 * (resolution < 256).  Results are bit-identical to the full forward. */
int dfot_uvit_forward_cached_masks(dfot_uvit_t h, const float* x, const float* noise_levels, float* out, int batch,
                                   const uint8_t* live_frames, const uint8_t* fresh_frames, void* stream);
/* debug/parity taps: copy an internal activation after the last forward (fp32). names: "pose_emb0","down0","down1",
 * "down2","mid","up2","up1","up0" in the oracle's NCHW layout. */
int dfot_uvit_read_tap(dfot_uvit_t h, const char* name, float* out, size_t capacity_floats, void* stream);

/* ---- pose-free U-ViT (the reference's UViT3D, algorithms/dfot/backbones/u_vit/u_vit3d.py:22-335) ----------------------------
 * UViT3DPose's parent class: the same U-Net, but the embedding every block's FiLM reads is a per-frame vector only,
 *   emb[b,t] = noise_level_pos_embedding(k[b,t]) (+ external_cond_embedding(cond[b,t]), zeroed for masked videos),
 * so there is no pose patch embedding, no set_conditions step, no per-window FiLM cache and no per-window state.  The geometry
 * fields mean what they mean in dfot_uvit_config and carry the same limits (head dim 64 or 128 at both transformer levels, ResBlock
 * channels multiples of 128, coarsest-level tokens a multiple of 128, RoPE, Fourier noise embedding); emb_channels, noise_dim <= 1024. */
typedef struct {
  int32_t channels[4];
  int32_t emb_channels;
  int32_t num_updown_blocks[3];
  int32_t num_mid_blocks;
  int32_t num_heads;
  int32_t in_channels;
  int32_t resolution;
  int32_t max_tokens;
  int32_t cond_dim;      /* external_cond_dim of the action embedding Linear(cond_dim, E) - SiLU - Linear(E, E); 0 = none; <= 1024 */
  int32_t noise_dim;     /* 256 */
  float rope_theta;
  float eps;
  int32_t cond_dropout;  /* non-zero: external_cond_dropout > 0 -- the keys are external_cond_embedding.embedding.linear_*, and
                          * external_cond_mask is honoured; zero: external_cond_embedding.linear_*, the mask is ignored (embeddings.py:364-387) */
} dfot_uvit3d_config;
/* The handle is a dfot_uvit_t: inventory (keys in the reference's state_dict() order: up_blocks before mid_blocks), load_weight, finalize,
 * reserve, workspace_bytes, set_option, query, attn_timing, read_tap (also "nemb": the per-frame embedding [B*T][E]; no "pose_emb0") and
 * destroy are the dfot_uvit_* calls above.  dfot_uvit_set_conditions / dfot_uvit_forward* refuse such a handle (DFOT_ERR_STATE), and
 * dfot_uvit3d_forward* refuse a pose handle. */
int dfot_uvit3d_create(const dfot_uvit3d_config* cfg, dfot_uvit_t* out);
int64_t dfot_uvit3d_config_bytes(void);  /* sizeof(dfot_uvit3d_config), for binding checks */
/* out[B,T,C,H,W] = model(x, noise_levels[B,T] fp32, external_cond[B,T,cond_dim] fp32 or NULL, external_cond_mask[B] bytes or NULL).
 * NULL external_cond: the noise embedding alone (unconditioned video).  external_cond on a model of cond_dim 0: DFOT_ERR_ARG. */
int dfot_uvit3d_forward(dfot_uvit_t h, const float* x, const float* noise_levels, const float* external_cond,
                        const uint8_t* external_cond_mask, float* out, int batch, void* stream);
/* ... with live_frames as in dfot_uvit_forward_cached_live (device uint8 [batch * T] or NULL): the frame-local tail skips dead frames */
int dfot_uvit3d_forward_live(dfot_uvit_t h, const float* x, const float* noise_levels, const float* external_cond,
                             const uint8_t* external_cond_mask, float* out, int batch, const uint8_t* live_frames, void* stream);
/* The inference engine's FiLM norm kernels at op level.  h / out: bf16 [bt*pixels][c]; stats [bt][32][2] = (mean, rstd); sv fp32
 * [bt][2c] and fcache bf16 [rows][2c] in the engine's column order (per 64 columns: 32 scale, then the 32 matching shift columns);
 * cond_mask: NULL or one byte per video of `tokens` frames.  fcache == NULL runs the pose-free instantiation (FiLM from sv alone; cond_mask is
 * not read). */
int dfot_op_gn_film_silu(const void* h, const float* stats, const float* gamma, const float* beta, const void* fcache, const float* sv,
                         const uint8_t* cond_mask, void* out, int bt, int pixels, int c, int tokens, void* stream);
/* x / out: bf16 [m][c], w fp32 [c]: out = RMSNorm(x) * w * (1 + scale) + shift */
int dfot_op_rms_film(const void* x, const float* w, const void* fcache, const float* sv, const uint8_t* cond_mask, void* out, int64_t m,
                     int c, int rows_per_bt, int tokens, float eps, void* stream);

/* ---- DiT3D backbone (Kinetics-600 path) --------------------------------------------------------------------- */
typedef struct dfot_dit_s* dfot_dit_t;

/* Hyper-parameters of dit3d (configurations/algorithm/backbone/dit3d.yaml:1-9 overridden by shortcut/DiT/XL.yaml and
 * dataset_experiment/kinetics_600_video_generation.yaml:22-23): variant "full", pos_emb_type "rope_3d", no external
 * condition, no causal mask. */
typedef struct {
  int32_t hidden_size;   /* 1152 */
  int32_t depth;         /* 28 */
  int32_t num_heads;     /* 16 (head dim 72) */
  int32_t patch_size;    /* 1 */
  int32_t in_channels;   /* 16 latent channels */
  int32_t height;        /* x_shape[1], 16 */
  int32_t width;         /* x_shape[2], 16 */
  int32_t max_tokens;    /* temporal length of the RoPE grid, 5 */
  int32_t mlp_hidden;    /* int(hidden*spatial_mlp_ratio); 0 = attention-only blocks (dit3d.yaml leaves it unset) */
  int32_t noise_dim;     /* 256 (sinusoidal Timesteps channels) */
  int32_t timesteps;     /* number of discrete noise levels, 1000 */
  float rope_theta;      /* 10000 */
  float eps;             /* 1e-6 (LayerNorm) */
  /* variant 0: DiT3D "full" + rope_3d (fields below ignored).
   * variant 1: DifferenceDiT3D "factorized_matrix_attention" + sinusoidal_2d, merge_type "interleaved" (the bash/k600 model,
   *   configurations/algorithm/backbone/difference_dit3d_factorized_matrix.yaml + shortcut/FacMatDiT/group_XL/XL-64-1.yaml):
   *   per depth one per-frame spatial DiTBlock (num_heads heads, MLP mlp_hidden) and one MatrixDiTBlock whose attention
   *   treats every frame as ONE token (a P x hidden matrix projected by left/right factors, dit_blocks.py:211-350);
   *   max_tokens counts the merged (difference, frame) tokens = 2 x the algorithm's max_tokens; hidden_size = embed_row_dim
   * variant 2: DiT3D "factorized_attention" + sinusoidal_factorized (configurations/algorithm/backbone/dit3d_factorized_attention.yaml
   *   + shortcut/FacDiT; dit_base.py:197-226,364-417): per depth one per-frame spatial DiTBlock (MLP mlp_hidden, 0 = none) and one
   *   temporal DiTBlock (MLP temporal_mlp_hidden, 0 = none) whose attention runs over the T frames of one patch position; the 2-D
   *   sinusoidal table is added at the patch embedding, the 1-D temporal table [max_tokens][hidden] after spatial block 0.
   *   Uses hidden_size, num_heads, mlp_hidden, temporal_mlp_hidden; (H/p)*(W/p) % 128 == 0, or == 64 with an even max_tokens
   *   (the per-frame attention is then dfot_op_attention_seq64's kernel, in training its backward dfot_op_attention_seq64_bwd[_packed]);
   *   max_tokens <= 32.  Trained through dfot_facdit_train_create; dfot_dit_train_create[_f] refuse it.
   * variant 3: DiT3D "factorized_matrix_attention" + sinusoidal_2d (FacMatDiT: configurations/algorithm/backbone/
   *   dit3d_factorized_matrix.yaml + shortcut/FacMatDiT): the block sequence and parameters of variant 1 without the difference front
   *   end -- no diff_embedder, the conditioning depends on the noise level only, max_tokens is the caller's (<= 32, odd counts
   *   allowed) -- and with use_temporal_rope the RoPE-1D over the frame axis (dit_base.py:297-306) on q and k of the matrix attention;
   *   the (cos, sin) table [max_tokens][hd/2] is built in float64 at create time and is not a parameter.  (H/p)*(W/p) % 128 == 0, or
   *   == 64 with an even max_tokens and even token counts (inference only; variant 1 keeps % 128).  embed_col_dim: a multiple of 64
   *   (left factors as GEMMs between per-frame transposes) or 1 .. 32 (inference only: the streaming kernels of
   *   dfot_op_facmat_contract / dfot_op_facmat_expand, no transposes); variant 1 keeps multiples of 64.  Trained through
   *   dfot_facmat_train_create; dfot_dit_train_create[_f] refuse it. */
  int32_t variant;
  int32_t embed_col_dim;        /* 64 */
  int32_t num_col_heads;        /* 1 */
  int32_t num_row_heads;        /* 16 */
  int32_t temporal_mlp_hidden;  /* int(hidden * mlp_ratio) of the matrix blocks (variant 1) / temporal blocks (variant 2), 4608 */
  int32_t use_bias;             /* qkv_bias / proj_bias of MatrixAttention present */
  /* external condition (BaseBackbone._build_external_cond_embedding, base_backbone.py:42-62; dmlab / minecraft: action, cond_ucf_101:
   * label).  DFOT_COND_NONE registers exactly the parameters of a model without these fields.
   *   action: external_cond_embedding[.embedding].linear_{1,2}.{weight,bias} = Linear(cond_dim, hidden) -> SiLU -> Linear(hidden, hidden);
   *           the ".embedding" level exists when cond_dropout != 0 (RandomDropoutCondEmbedding, embeddings.py:364-387)
   *   label:  external_cond_embedding.embedding_table.weight [num_classes + (cond_dropout != 0)][hidden] (the extra row is the null class) */
  int32_t cond_type;     /* DFOT_COND_NONE / DFOT_COND_ACTION / DFOT_COND_LABEL */
  int32_t cond_dim;      /* action: values per (video, token) */
  int32_t num_classes;   /* label */
  int32_t cond_dropout;  /* cfg.external_cond_dropout > 0 */
  int32_t use_temporal_rope;  /* variant 3: RoPE-1D over the frame axis on q and k of the matrix attention (0: none; other variants ignore it) */
} dfot_dit_config;
enum { DFOT_COND_NONE = 0, DFOT_COND_ACTION = 1, DFOT_COND_LABEL = 2 };

/* dfot_dit_config with one trailing field, as its own type: dfot_dit_config keeps its size and its last field, so callers built against
 * it (and dfot_dit_create / dfot_dit_train_create, which read exactly that many bytes) stay valid.
 * fourier_noise = backbone.use_fourier_noise_embedding (ContinuousDiffusion, shortcut/diffusion/continuous.yaml): the noise level is a float
 * (precond_scale * logsnr) embedded by FourierEmbedding (embeddings.py:94-109) -> TimestepEmbedding.  Registers the two persistent buffers
 * noise_level_pos_embedding.timesteps.{freqs,phases} [noise_dim] before embedding.linear_1 (the reference's state_dict position), builds
 * no per-level table, and is driven through the *_forward_f entry points only.  0: exactly the model dfot_dit_create builds from `base`. */
typedef struct {
  dfot_dit_config base;
  int32_t fourier_noise;
} dfot_dit_config_f;

int dfot_dit_create(const dfot_dit_config* cfg, dfot_dit_t* out);
int dfot_dit_create_f(const dfot_dit_config_f* cfg, dfot_dit_t* out);
int dfot_dit_destroy(dfot_dit_t h);
int dfot_dit_num_params(dfot_dit_t h);
const char* dfot_dit_param_name(dfot_dit_t h, int index);
int dfot_dit_param_shape(dfot_dit_t h, int index, int64_t shape[4], int* ndim);
int dfot_dit_load_weight(dfot_dit_t h, const char* name, const float* data, const int64_t* shape, int ndim, void* stream);
/* verify every key was loaded; build the RoPE table and the noise-level modulation table: the conditioning of this
 * backbone is a function of the integer noise level alone, so every AdaLN shift/scale/gate of every block is
 * evaluated for all `timesteps` levels once (one GEMM) and forward only indexes it */
int dfot_dit_finalize(dfot_dit_t h, void* stream);
int dfot_dit_reserve(dfot_dit_t h, int max_batch);
size_t dfot_dit_workspace_bytes(dfot_dit_t h);
/* "gemm_variant" (-1 auto), "time_attn" (as for dfot_uvit_set_option), "front_only" (1: a forward stops once the AdaLN modulations
 * of the call are formed and leaves `out` untouched -- for timing the front end alone) */
int dfot_dit_set_option(dfot_dit_t h, const char* key, int value);
int dfot_dit_attn_timing(dfot_dit_t h, double* total_ms, int64_t* launches);
/* out[B,T,C,H,W] = model(x[B,T,C,H,W], noise_levels[B,T]) ; x/out fp32, noise_levels int32 in [0, timesteps)
 * (device pointer; out-of-range levels are clamped), T <= max_tokens with T*(H/p)*(W/p) % 128 == 0.
 * variant 1: x holds the interleaved (difference_0, frame_0, difference_1, ...) tokens, T even, (H/p)*(W/p) % 128 == 0.
 * variant 2: any 1 <= T <= max_tokens (the temporal table's first T rows are used), (H/p)*(W/p) % 128 == 0; variants 2 and 3 at
 * (H/p)*(W/p) == 64: even T only (the rule of the first line). */
int dfot_dit_forward(dfot_dit_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens,
                     void* stream);
/* The same forward with an external condition per (video, token): `cond` fp32 [B,T,cond_dim] (action models) or `labels` int32 [B,T]
 * (label models; rows outside the table are clamped), the other one NULL.  One kernel forms e = noise-level embedding (+ token kind,
 * variant 1) + condition embedding per frame; videos whose `cond_mask` byte [B] is set (NULL: none) keep e without the condition and
 * produce bit-for-bit the output of dfot_dit_forward.  The AdaLN modulations of the frames come from one GEMM over e instead of the
 * per-level table; nothing after that differs.  No allocation, no host synchronisation: capturable in a graph. */
int dfot_dit_forward_cond(dfot_dit_t h, const float* x, const int32_t* noise_levels, const float* cond, const int32_t* labels,
                          const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream);
/* Continuous diffusion (a model of dfot_dit_create_f with fourier_noise != 0): out = model(x, noise_levels[B,T] fp32).  One kernel forms, per frame and in fp32,
 * feat[j] = sqrt(2) * cos(level * freqs[j] + phases[j]) (one rounded multiply, one rounded add, accurately range-reduced cosine) and
 * n = linear_2(SiLU(linear_1(feat))); e = n (+ token kind, variant 1) (+ condition embedding unless the video's cond_mask byte is set) then
 * feeds the per-frame modulation GEMM of dfot_dit_forward_cond, and nothing after it differs.  cond / labels / cond_mask as in
 * dfot_dit_forward_cond; all NULL runs without a condition term (the only form an unconditioned model takes).  No allocation, no host
 * synchronisation; a video gives the same bits alone and in a batch.  On a model without fourier_noise this returns DFOT_ERR_ARG, as
 * dfot_dit_forward / dfot_dit_forward_cond do on a model with it. */
int dfot_dit_forward_f(dfot_dit_t h, const float* x, const float* noise_levels, const float* cond, const int32_t* labels,
                       const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream);
/* parity taps after the last forward: "emb" [timesteps][hidden] (noise-level embedding of every level; DFOT_ERR_ARG on a fourier_noise
 * model, which tabulates nothing), "stream" [B*T*P][hidden] (residual stream after the last block), "cond_emb" [B*T][hidden] (e of the
 * last per-frame forward), "noise_feat" [B*T][noise_dim] (Fourier features of the last dfot_dit_forward_f) */
int dfot_dit_read_tap(dfot_dit_t h, const char* name, float* out, size_t capacity_floats, void* stream);
/* The DiT final layer alone (test / benchmark entry of the launch both engines make): out [frames][c][h][w] fp32 = unpatchify(Linear(
 * LayerNorm(x) * (1 + scale) + shift)) for x [rows][hidden] fp32, rows = frames * rows_per_frame, rows_per_frame = (h / patch) * (w / patch),
 * (shift | scale) = table[clamp(levels[frame], 0, max_level)][off .. off + 2 * hidden) with table rows of ldt floats, weight [patch * patch * c]
 * [hidden] fp32 with the output index (py, px, channel), channel fastest, bias [patch * patch * c].  hidden: a LayerNorm kernel width <= 2048;
 * patch * patch * c <= 256.  form 0: the engine's own choice (the LDS-resident kernel whenever the weight fits in 160 KiB, else the chunked
 * one); 1: the LDS-resident kernel, DFOT_ERR_SHAPE if the weight does not fit; 2: the chunked kernel, which streams floor(160 KiB / (4 *
 * hidden)) weight rows at a time through LDS.  Both kernels add an output's products in the same order: the same bits. */
int dfot_op_dit_final_layer(const float* x, const float* table, const int32_t* levels, int64_t ldt, int64_t off, const float* w, const float* b,
                            float* out, int hidden, int rows_per_frame, int rows, float eps, int max_level, int c, int h, int width, int patch,
                            int form, void* stream);
/* the chunked kernel with `chunk` (> 0, at most what fits) weight rows per pass: lets a test split a small weight as a large one splits */
int dfot_op_dit_final_layer_chunked(const float* x, const float* table, const int32_t* levels, int64_t ldt, int64_t off, const float* w,
                                    const float* b, float* out, int hidden, int rows_per_frame, int rows, float eps, int max_level, int c, int h,
                                    int width, int patch, int chunk, void* stream);

/* ---- single launches of the DiT / DiT1D block kernels (test entries) ----
 * Each runs the launcher function the engines call (same grid, block and argument order) on buffers the caller provides; nothing is
 * allocated except the grow-only partial-sum scratch of the deterministic sums.  Conventions: x / dx / dy / dm [rows][hidden] fp32,
 * rows = frames * rows_per_frame; `bf16` buffers are [rows][hidden] unless stated; a modulation table has rows of ldt floats and the op's
 * columns start at `off` (ldt and off multiples of 4).  ln_mod and dit1d_ln_share index the table by clamp(levels[frame], 0, max_level);
 * the training ops (gate_combine, gate_bwd, ln_bwd) take the trainer's per-frame table: row f belongs to frame f.
 * Refused by name: a hidden size without a LayerNorm kernel instance (DFOT_ERR_SHAPE), rows_per_frame % 4 != 0 for gate_bwd / ln_bwd,
 * hidden % 4 != 0, head dim or packed row length not multiples of 8, patch * patch * c > 256, null pointers. */
/* xout [rows][hidden] fp32 and obf bf16 <- LayerNorm(xin) * (1 + scale) + shift; xout may be xin; (shift | scale) at off */
int dfot_op_dit_ln_mod(const float* xin, float* xout, void* obf, const float* table, const int32_t* levels, int64_t ldt, int64_t off, int hidden,
                       int rows_per_frame, int rows, float eps, int max_level, void* stream);
/* y = x + gate[frame] * a (a bf16), gate = table[frame][off .. off + hidden) */
int dfot_op_dit_gate_combine(const float* x, float* y, const void* a, const float* table, int64_t ldt, int64_t off, int hidden, int rows_per_frame,
                             int rows, void* stream);
/* da bf16 = dy * gate; dbias [hidden] = sum over all rows of da (as stored, bf16); dmod[frame][off + c] = sum over the frame's rows of dy * a.
 * dmod_part [4][frames][ldt]: the kernel stores the gate's hidden columns of every plane; dbias_part [4 * frames][hidden];
 * dmod [frames][ldt] = the four planes of dmod_part added in a fixed order, every column (what the caller left in the others included) */
int dfot_op_dit_gate_bwd(const float* dy, const void* a, const float* table, int64_t ldt, int64_t off, void* da, float* dmod_part, float* dbias_part,
                         float* dbias, float* dmod, int hidden, int rows_per_frame, int frames, void* stream);
/* backward of m = LayerNorm(x) * (1 + scale) + shift for dm: dx [rows][hidden], stats [rows][2] = (mean, rstd), and through dmod_part / dmod (as
 * gate_bwd) dshift at columns [off, off + hidden) and dscale at [off + hidden, off + 2 * hidden); scale = table[frame][off + hidden ...) */
int dfot_op_dit_ln_bwd(const float* dm, const float* x, const float* table, int64_t ldt, int64_t off, float* dx, float* stats, float* dmod_part,
                       float* dmod, int hidden, int rows_per_frame, int frames, float eps, void* stream);
/* the row part of ln_bwd alone (dx and stats), any rows_per_frame */
int dfot_op_dit_ln_bwd_rows(const float* dm, const float* x, const float* table, int64_t ldt, int64_t off, float* dx, float* stats, int hidden,
                            int rows_per_frame, int frames, float eps, void* stream);
/* tanh-GELU on n bf16 elements (n % 8 == 0): h = gelu(u) when h is given; dh_to_du *= gelu'(u) in place when it is given */
int dfot_op_dit_gelu(const void* u, void* h, void* dh_to_du, int64_t n, void* stream);
/* PatchEmbed (Conv2d, kernel = stride = patch): x [frames][c][h][width] -> out [rows][hidden], w [hidden][c * patch * patch], pos [rows per
 * frame][hidden] or NULL; its data gradient dx [frames][c][h][width] from dy [rows][hidden]; its weight gradients dw += , db += */
int dfot_op_dit_patch_embed(const float* x, const float* w, const float* b, const float* pos, float* out, int c, int h, int width, int patch,
                            int hidden, int64_t rows, void* stream);
int dfot_op_dit_patch_embed_dgrad(const float* dy, const float* w, float* dx, int c, int h, int width, int patch, int hidden, int64_t rows,
                                  void* stream);
int dfot_op_dit_patch_embed_wgrad(const float* dy, const float* x, float* dw, float* db, int c, int h, int width, int patch, int hidden, int64_t rows,
                                  void* stream);
/* dout [frames][c][h][width] fp32 gathered per token: dyp [rows][ocp] bf16 (columns (py, px, channel) < patch * patch * c written) and its
 * transpose dyt [..][rows] (rows < patch * patch * c written); the caller zeroes the padding */
int dfot_op_dit_final_gather(const float* dout, void* dyp, void* dyt, int64_t rows, int c, int h, int width, int patch, int ocp, void* stream);
/* (dq, dk, dv) [rows / ntok][heads][ntok][dstride] bf16 -> out [rows][3 * heads * d] (q | k | v, head-major); with rope_cs [ntok][d / 2][2]
 * (cos, sin) dq and dk are rotated by the transpose of the forward rotation */
int dfot_op_dit_qkv_grad_pack(const void* dq, const void* dk, const void* dv, const float* rope_cs, void* out, int64_t rows, int ntok, int heads, int d,
                              int dstride, void* stream);
/* DiT1D: X [rows][hidden] = w x + b + pos for x [frames][C][L] (channel-major frames), rows = videos * n, n tokens per video, pos [n][hidden] */
int dfot_op_dit1d_tok_embed(const float* x, const float* w, const float* b, const float* pos, float* X, int C, int L, int n, int hidden, int64_t rows,
                            void* stream);
/* DiT1D share_norm: X <- LayerNorm(X) in place, A bf16 <- LayerNorm(X) * (1 + scale) + shift; idx [frames] int32 receives the clamped levels */
int dfot_op_dit1d_ln_share(float* X, void* A, const float* table, const int32_t* levels, int32_t* idx, int64_t ldt, int64_t off, int hidden,
                           int rows_per_frame, int rows, float eps, int max_level, void* stream);
/* DiT1D final layer: out [frames][C][L] = Linear(LayerNorm(X)), w [C][hidden] */
int dfot_op_dit1d_final(const float* X, const float* w, const float* b, float* out, int hidden, int C, int L, int rows, float eps, void* stream);
/* DiT1D training kernels (csrc/dit1d_train.hip).  All fp32, fixed-order sums: two calls on the same inputs give the same bits.
 * share_norm LayerNorm with saved statistics, not in place: N [rows][hidden] = LayerNorm(X), rstd [rows], M bf16 = N * (1 + scale) + shift
 * with (shift | scale) = table[row / rows_per_frame][off, off + 2 * hidden): one table row per frame */
int dfot_op_dit1d_ln_share_train(const float* X, float* N, float* rstd, void* M, const float* table, int64_t ldt, int64_t off, int hidden,
                                 int rows_per_frame, int rows, float eps, void* stream);
/* its backward.  The residual base of a share_norm block is N itself, so two gradients arrive: dres [rows][hidden] over the residual path and
 * dm [rows][hidden] of the modulated GEMM operand.  dn = dres + dm * (1 + scale); dx = rstd * (dn - mean(dn) - N * mean(dn * N));
 * dmod_part [4][frames][ldt]: plane z receives, at columns [off, off + hidden) and [off + hidden, off + 2 * hidden), the sums of dm and of
 * dm * N over rows [z, z + 1) * rows_per_frame / 4 of every frame (rows_per_frame % 4 == 0; dres enters neither).  dm == NULL is the final
 * layer's LayerNorm: dn = dres, table and dmod_part are not used.  dx may be dres. */
int dfot_op_dit1d_ln_share_bwd(const float* dres, const float* dm, const float* N, const float* rstd, const float* table, int64_t ldt, int64_t off,
                               float* dx, float* dmod_part, int hidden, int rows_per_frame, int frames, void* stream);
/* backward of dfot_op_dit1d_final for dout [frames][C][L]: dx [rows][hidden] (d nf = dout * w goes through the LayerNorm backward without
 * being stored), stats [rows][2] = (mean, rstd) of X's rows, dW [C][hidden] = sum over the rows of dout * LayerNorm(X), db [C] = sum of dout.
 * part: workspace of ceil(rows / 64) * C * (hidden + 1) floats (the sums of 64 rows each, then added in their order) */
int dfot_op_dit1d_final_bwd(const float* dout, const float* X, const float* w, float* dx, float* stats, float* part, float* dW, float* db, int hidden,
                            int C, int L, int rows, float eps, void* stream);
/* backward of dfot_op_dit1d_tok_embed for dX0 [rows][hidden], weights: dW [hidden][C] = sum over the rows of dX0 * x[(frame, c, l)],
 * db [hidden] = sum of dX0 (pos is a frozen buffer: nothing is computed for it).  part: ceil(rows / 64) * (C + 1) * hidden floats */
int dfot_op_dit1d_tok_embed_wgrad(const float* dX0, const float* x, float* part, float* dW, float* db, int C, int L, int hidden, int64_t rows,
                                  void* stream);
/* ... and input: dx [frames][C][L] = dX0 * w, w [hidden][C] */
int dfot_op_dit1d_tok_embed_dgrad(const float* dX0, const float* w, float* dx, int C, int L, int hidden, int64_t rows, void* stream);

/* ---- attention maps (the read-out of the reference's attn_hook: algorithms/common/attn_hook/hook.py, dit_blocks.py:100-118) ----
 * Which frame attends to which, per head, of the blocks whose attention mixes frames: the blocks of variant 0 (full 3-D attention), the
 * temporal blocks of variant 2 and the matrix blocks of variant 3.  The forward kernels never form the score matrix; with a capture on,
 * every selected block adds one map launch (plus its finalize) to dfot_dit_forward* on the caller's stream, which recomputes the
 * softmax from the q and k (bf16, after RoPE, pre-scaled) the block's attention kernel read.  Off (the default): no launch, no buffer.
 *   frame form: F[b][head][tq][tk] = (1/P) sum_{i in frame tq} sum_{j in frame tk} softmax_j(q_i . k_j); rows sum to 1.
 *               variant 0 / 2: [batch][num_heads][T][T];  variant 3: [batch][num_col_heads][num_row_heads][T][T]
 *   full form:  variant 0: A [batch][num_heads][T*P][T*P];  variant 3: every frame is one token, so the full map is the frame map;
 *               variant 2: refused (DFOT_ERR_ARG): a temporal block has one T x T map per patch position and only their mean is formed. */
enum { DFOT_ATTN_MAP_OFF = -1, DFOT_ATTN_MAP_FRAME = 0, DFOT_ATTN_MAP_FULL = 1 };
/* Select the blocks (`count` ascending indices into the variant's frame-mixing blocks, each < depth; blocks == NULL: all of them) and the
 * form; form DFOT_ATTN_MAP_OFF releases the buffers and turns the capture off.  The buffers (one map per selected block at max_batch x
 * max_tokens) are allocated here when a workspace is reserved and in every later dfot_dit_reserve.  max_bytes (0: 1 GiB) caps them: a
 * capture that needs more is refused with DFOT_ERR_SHAPE and a message naming the size -- here (the earlier setting stays), or in the
 * dfot_dit_reserve that would grow them (the workspace stays as it was).  Variant 1 (the difference model) is refused with DFOT_ERR_ARG.  Synchronises the device; not for use during graph capture. */
int dfot_dit_capture_attention(dfot_dit_t h, const int32_t* blocks, int count, int form, size_t max_bytes);
/* shape (ndim <= 5) of the map of selected block `slot` (0 .. count-1) as the last forward wrote it; DFOT_ERR_STATE until a forward has
 * run with the capture on */
int dfot_dit_attention_map_shape(dfot_dit_t h, int slot, int64_t shape[5], int* ndim);
/* copy that map (fp32, device to device, on `stream`); same DFOT_ERR_STATE rule */
int dfot_dit_read_attention_map(dfot_dit_t h, int slot, float* out, size_t capacity_floats, void* stream);

/* ---- DiT3D training path ("full" variant, attention-only blocks) ----------------------------------
 * Replaces torch autograd through DiT3D.forward (algorithms/dfot/backbones/dit/dit3d.py:153-192, dit_blocks.py:408-542) and the
 * optimizer step of DFoTVideo.training_step / configure_optimizers (dfot_video.py:41-75, base_pytorch_algo: AdamW).
 * Parameters, gradients and optimizer moments live in caller-owned flat fp32 buffers (reference state_dict order, every
 * tensor 16-byte aligned at dfot_dit_train_param_offset) so a data-parallel job all-reduces ONE buffer.
 *   create -> attach(params, grads) -> [copy weights into params] -> reserve(batch) -> sync_weights
 *   step: forward(x_t, levels) -> loss + dfot_vloss_grad -> backward(d_out) -> [all-reduce grads] -> dfot_sumsq + dfot_adamw_step
 *         -> sync_weights */
typedef struct dfot_dit_train_s* dfot_dit_train_t;
int dfot_dit_train_create(const dfot_dit_config* cfg, dfot_dit_train_t* out);
int dfot_dit_train_create_f(const dfot_dit_config_f* cfg, dfot_dit_train_t* out);  /* with dfot_dit_config_f.fourier_noise (see dfot_dit_create_f) */
/* trainer of the DiT3D factorized-matrix model (FacMatDiT: variant 3 only, any other variant: DFOT_ERR_ARG; fourier_noise != 0:
 * DFOT_ERR_ARG).  The handle is a dfot_dit_train_t: every other dfot_dit_train_* function takes it.  Parameters in the reference's
 * registration order (no diff_embedder), any 1 <= T <= max_tokens <= 32 (odd frame totals included), the temporal RoPE table built in
 * float64 when use_temporal_rope is set; actions / labels through dfot_dit_train_forward_cond.  dfot_dit_train_create[_f] keep refusing
 * variant 3 and name this function. */
int dfot_facmat_train_create(const dfot_dit_config_f* cfg, dfot_dit_train_t* out);
/* dfot_facmat_train_create that also builds (H/p)*(W/p) == 64, the taichi res-128 facmat-s-{64-1,64-4,64-16,128-1}-bias recipes (variant 3
 * only, embed_col_dim 64 or 128 as there; any other variant or fourier_noise != 0: DFOT_ERR_ARG).  At 64 patches max_tokens must be even
 * (an odd one: DFOT_ERR_SHAPE) and so must T: dfot_dit_train_forward[_cond] refuse an odd T with DFOT_ERR_SHAPE before they launch
 * anything, so the gradients of the previous step stay as they were.  The spatial blocks then run dfot_op_attention_seq64's kernel and
 * dfot_op_attention_seq64_bwd_packed's, the matrix block's forward is unchanged, and the gradients of the two left factors qkv_u / proj_u
 * go through dfot_op_facmat_factor_wgrad's launcher, straight into the gradient buffer.  At a multiple of 128 patches it builds exactly
 * what dfot_facmat_train_create builds (the same gradient bits).  A separate entry because dfot_facmat_train_create is held to its
 * refusal of 64 patches. */
int dfot_facmat_train_create_p64(const dfot_dit_config_f* cfg, dfot_dit_train_t* out);
/* trainer of the DiT3D factorized-attention model (FacDiT: variant 2 only, any other variant: DFOT_ERR_ARG; fourier_noise != 0:
 * DFOT_ERR_ARG).  The handle is a dfot_dit_train_t: every other dfot_dit_train_* function takes it.  Parameters in the reference's
 * registration order (all spatial blocks, then all temporal blocks), executed spatial i, temporal i; any 1 <= T <= max_tokens <= 32 (the
 * first T rows of the temporal sinusoidal table, which is built at create time and is not a parameter); (H/p)*(W/p) % 128 == 0, MLP
 * widths multiples of 128, head dim a multiple of 8; actions / labels through dfot_dit_train_forward_cond.  dfot_dit_train_create[_f]
 * keep refusing variant 2 and name this function.
 * (H/p)*(W/p) == 64 (the taichi res-128 recipes) also trains when max_tokens is even (an odd one: DFOT_ERR_SHAPE), with even T only: the
 * forward refuses T x 64 rows that are no multiple of 128 with DFOT_ERR_SHAPE before it launches anything.  The spatial blocks then run
 * dfot_op_attention_seq64's kernel and, backward, dfot_op_attention_seq64_bwd_packed's (nothing but q, k, v is kept for it). */
int dfot_facdit_train_create(const dfot_dit_config_f* cfg, dfot_dit_train_t* out);
/* MEASUREMENT HOOK, not a supported option (it exists so that tools/bench_ops.py can time both forms on one handle, and may go once the
 * three-buffer form is no longer worth comparing).  A variant 2 handle at 64 patches per frame: packed != 0 (the default) runs the spatial blocks' attention backward as ONE launch that
 * stores dq | dk | dv into the packed gradient rows; 0 runs dfot_op_attention_seq64_bwd's form followed by the pack kernel.  The gradient
 * bits are the same; the switch exists so that the two forms can be timed in one process.  No effect at other patch counts. */
int dfot_facdit_train_set_seq64_packed(dfot_dit_train_t h, int packed);
int dfot_dit_train_destroy(dfot_dit_train_t h);
int dfot_dit_train_num_params(dfot_dit_train_t h);
const char* dfot_dit_train_param_name(dfot_dit_train_t h, int i);
int dfot_dit_train_param_shape(dfot_dit_train_t h, int i, int64_t shape[4], int* ndim);
int64_t dfot_dit_train_param_offset(dfot_dit_train_t h, int i);
int64_t dfot_dit_train_total_numel(dfot_dit_train_t h);
size_t dfot_dit_train_workspace_bytes(dfot_dit_train_t h);
int dfot_dit_train_attach(dfot_dit_train_t h, float* params, float* grads);
int dfot_dit_train_reserve(dfot_dit_train_t h, int max_batch);
int dfot_dit_train_sync_weights(dfot_dit_train_t h, void* stream);
/* out = model(x, levels), saving what backward needs; x must stay valid until backward */
int dfot_dit_train_forward(dfot_dit_train_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens, void* stream);
/* dfot_dit_train_forward with the external condition (arguments as dfot_dit_forward_cond; cond_mask [B] is the per-video dropout mask the
 * caller drew).  cond / labels are copied: only x must stay valid until backward, which then also fills the gradients of the condition
 * embedding (label table: row-wise sums in frame order, rows of unused classes exactly zero; no floating-point atomics). */
int dfot_dit_train_forward_cond(dfot_dit_train_t h, const float* x, const int32_t* noise_levels, const float* cond, const int32_t* labels,
                                const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream);
/* fourier_noise models: freqs / phases are buffers, not parameters -- they are NOT part of the flat parameter / gradient / moment buffers
 * (no gradient, no optimizer state, no weight decay can reach them).  Load each once: name = the reference's state_dict key
 * ("noise_level_pos_embedding.timesteps.freqs" / ".phases"), data = device fp32 [noise_dim]. */
int dfot_dit_train_load_buffer(dfot_dit_train_t h, const char* name, const float* data, int64_t numel, void* stream);
/* dfot_dit_train_forward / _cond for a fourier_noise model: float levels [B,T]; cond / labels / cond_mask all NULL on an unconditioned
 * model (or to run without the condition term).  The backward is dfot_dit_train_backward, with the Fourier features as linear_1's input. */
int dfot_dit_train_forward_f(dfot_dit_train_t h, const float* x, const float* noise_levels, const float* cond, const int32_t* labels,
                             const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream);
/* grads <- d(sum(out * d_out))/d(params) for the last forward (overwrites the attached gradient buffer) */
int dfot_dit_train_backward(dfot_dit_train_t h, const float* d_out, void* stream);
/* dx[B,T,C,H,W] <- d(sum(out * d_out))/d(x) of the same forward / backward pair (call after dfot_dit_train_backward): what autograd gives
 * `x.grad` when x requires it -- reconstruction guidance differentiates the prediction w.r.t. x_t (discrete_diffusion.py:485-513) */
int dfot_dit_train_input_grad(dfot_dit_train_t h, float* dx, void* stream);
/* dv[B,T,F] = coef[b,t] * d/dv of the loss term of dfot_vspace_loss (vspace = 1) / dfot_vpred_loss (vspace = 0) */
int dfot_vloss_grad(const float* x, const float* noise, const float* v, const float* a, const float* sigma, const float* coef, float* dv,
                    int batch, int tokens, int64_t frame_elems, int vspace, void* stream);
/* out[0] = sum x^2 (device scalar) */
int dfot_sumsq(const float* x, int64_t n, float* out, void* stream);
/* torch.optim.AdamW on flat buffers; grad_sumsq (optional device scalar): clip the gradient to max_grad_norm first;
 * ema (optional): shadow = ema_decay * shadow + (1 - ema_decay) * new parameter, in the same pass (algorithms/common/ema.py:22-32) */
int dfot_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, const float* grad_sumsq, float max_grad_norm, float* ema, float ema_decay,
                    void* stream);

/* ---- camera-pose front end ------------------------------------------------------------------- */
/* raw poses [B,T,16] (fx,fy,px,py | 3x4 RT) -> ray encoding [B,T,180,res,res] fp32, normalised by frame 0 */
int dfot_ray_encode(const float* raw_poses, float* out, int batch, int tokens, int resolution, void* stream);
/* same encoding for poses the caller has already expressed in its world frame (no normalisation by frame 0): the options of
 * DFoTVideoPose._process_conditions off the default path -- normalize_by "mean", `bound`, and the interpolation of masked poses
 * under temporal History Guidance (dfot_video_pose.py:75-98, utils/geometry_utils.py:135-205) -- are a few 3x3 products per
 * frame and are done by the host (diffusion-forcing-transformer_amd/pose.py) before this call */
int dfot_ray_encode_normalized(const float* poses, float* out, int batch, int tokens, int resolution, void* stream);

/* ---- sampler step (per-step coefficient tables live in device memory) -------------------------- */
/* coef tables are [n_branch_batch = B*NFE][T] fp32, row-major, for ONE step:
 *   qa,qb : x_in = qa*x + qb*noise      (history token re-noising; (1,0) = keep)
 * x[B,T,F] fp32, noise[B*NFE,T,F] fp32 (may be NULL when every qb is 0), x_in[B*NFE,T,F] fp32. */
int dfot_hg_prepare(const float* x, const float* noise, const float* qa, const float* qb, float* x_in, int batch,
                    int nfe, int tokens, int64_t frame_elems, void* stream);
/* per (branch-batch,t): sa=sqrt(abar_k), s1=sqrt(1-abar_k), an=sqrt(abar_next), cn=sqrt(1-abar_next-sigma^2),
 * keep (curr==next) as 0/1 floats; weight[NFE]; gen[B,T] (1 = token being generated, 0 = context/padding).
 *   x0 = sa*x_in - s1*v ; eps = sa*v + s1*x_in ; x_pred = keep ? x_in : x0*an + eps*cn
 *   x_next[b,t] = gen ? sum_h weight[h]*x_pred[b*NFE+h,t] : x[b,t] */
int dfot_ddim_compose(const float* x, const float* x_in, const float* v, const float* sa, const float* s1,
                      const float* an, const float* cn, const float* keep, const float* weight, const uint8_t* gen,
                      float* x_next, int batch, int nfe, int tokens, int64_t frame_elems, void* stream);

/* same with weight[NFE][T]: one composition weight per (branch, token) -- History Guidance with several gen segments
 * (history_guidance.py:545-568: excluded gen tokens contribute 0, the sum is divided by the number of segments covering the token) */
int dfot_ddim_compose_tokw(const float* x, const float* x_in, const float* v, const float* sa, const float* s1,
                           const float* an, const float* cn, const float* keep, const float* weight, const uint8_t* gen,
                           float* x_next, int batch, int nfe, int tokens, int64_t frame_elems, void* stream);

/* stochastic part of a sampling step -- the `sigma * noise` term of ddim_sample_step for eta > 0
 * (algorithms/dfot/diffusion/discrete_diffusion.py:468-472,515-527) and the posterior-variance term of ddpm_sample_step
 * (:441-449; the DDPM mean is the dfot_ddim_compose form with an = coef1 + coef2*sa, cn = coef2*s1).  Composition is linear:
 *   x_next[b,t] += sum_h weight[h (,t)] * sigma[b*NFE+h,t] * noise[b*NFE+h,t]     where gen[b,t]
 * sigma[B*NFE][T] fp32 with 0 for kept tokens; noise[B*NFE,T,F] fp32, clamped by the caller; weight_per_token selects weight[NFE][T]. */
int dfot_ddim_noise(const float* noise, const float* sigma, const float* weight, const uint8_t* gen, float* x_next, int batch,
                    int nfe, int tokens, int64_t frame_elems, int weight_per_token, void* stream);

/* ---- denoising loss of one noised forward (training_step / validation denoising loss) -------------------------- */
/* replaces ContinuousDiffusion.forward's frame arithmetic (diffusion/continuous_diffusion.py:140-167):
 *   x_t = alpha*x + sigma*noise ; eps_hat = alpha*v + sigma*x_t ; loss[b,t] = mean_frame( weight*(eps_hat-noise)^2 ) ;
 *   x_pred = alpha*x_t - sigma*v (optional, may be NULL).  alpha/sigma/weight are [B*T] fp32 (host-computed from the
 *   cosine logSNR schedule); scratch holds dfot_vpred_loss_scratch_floats() floats.  v = backbone(x_t, 0.125*logsnr, cond). */
int dfot_vpred_loss(const float* x, const float* noise, const float* v, const float* alpha, const float* sigma,
                    const float* weight, float* x_pred, float* scratch, float* loss, int batch, int tokens,
                    int64_t frame_elems, void* stream);
int64_t dfot_vpred_loss_scratch_floats(int batch, int tokens, int64_t frame_elems);
/* DiscreteDiffusion.forward, objective pred_v (diffusion/discrete_diffusion.py:345-377): same inputs, but the error is taken
 * in v-space: loss[b,t] = mean_frame( weight * (v - (alpha*noise - sigma*x))^2 ); alpha/sigma = sqrt(abar_k), sqrt(1-abar_k) of the
 * token's integer level, weight = compute_loss_weights (min-SNR / fused min-SNR / sigmoid, host-computed, :274-343) */
int dfot_vspace_loss(const float* x, const float* noise, const float* v, const float* alpha, const float* sigma,
                     const float* weight, float* x_pred, float* scratch, float* loss, int batch, int tokens,
                     int64_t frame_elems, void* stream);

/* ---- unit-testable primitives ------------------------------------------------------------------ */
/* C[M,N] (fp32) = A[M,K] (bf16, row stride lda) * W[N,K]^T (bf16) + bias[N] (fp32 or NULL)
 * variant: -1 auto (pick by shape), 0 = 128x128 tile, register staging (independent reference), 1 = 128x128 LDS-DMA, 4 = 256x256
 * (16 waves), 6 = 512x128 (16 waves), 8 = 128x128 with K split inside the workgroup, 9 = 256x192, 10 = 128x192, 14 = 256x144 three-stage
 * ring; the 256-row forms need M % 256 == 0 (512 for 6).  Other numbers: DFOT_ERR_ARG */
int dfot_op_gemm(const void* a_bf16, int lda, const void* w_bf16, const float* bias, float* c, int m, int n, int k,
                 int variant, void* stream);
/* y[BT,H,W,Cout] (fp32) = conv3x3(pad 1)(a[BT,H,W,Cin] bf16, w[Cout][9*Cin] bf16 tap-major) + bias */
int dfot_op_conv3x3(const void* a_bf16, const void* w_bf16, const float* bias, float* y, int bt, int h, int w,
                    int cin, int cout, int variant, void* stream);
/* Test entry to the whole GEMM / implicit-GEMM launcher with every fused epilogue.  The fields mirror the engine's internal
 * argument block one to one (amode 0 = dense A, 1 = conv3x3; epi 0 = fp32, 1 = bf16, 2 = fused attention+MLP projection,
 * 3 = DiT q|k|v; variant as for the plain GEMM entry); their meaning is documented at that block.  Pointers are device pointers
 * or NULL; the conv zero page is supplied by the library.  The launcher's own checks are the only validation. */
typedef struct {
  int32_t amode, epi, variant;
  const void* A; int64_t lda;
  const void* W; int64_t ldw;
  int32_t M, N, K, H, Wd, Cin;
  const uint8_t* live;
  const float* bias; int32_t bias_rows;
  float* out_f32; void* out_bf16; int64_t ldo;
  const float* resid; const void* resid_bf;
  const float* gate; const int32_t* gate_index; int64_t ldg; int32_t gate_rows;
  int32_t act; void* pre_act; void* raw; int64_t ldraw; int32_t tr_rows;
  float* gn_part; int32_t gn_rows_per_bt, gn_cpg;
  void* out2; int64_t ldo2; int32_t split;
  void *q, *k, *v;
  const float *qw, *kw, *rope_cs;
  int32_t heads, d, ntok; float qscale; int32_t dstride; float eps;
  int32_t ksplit; int64_t slice_stride;
} dfot_gemm_desc;
int dfot_op_gemm_ex(const dfot_gemm_desc* desc, void* stream);
/* sizeof(dfot_gemm_desc): the Python mirror of the struct checks its layout against it */
int64_t dfot_op_gemm_desc_bytes(void);
/* o[B,N,heads*d] (bf16, row stride ldo) = softmax(q k^T) v ; q,k,v [B,heads,N,d] bf16; q pre-scaled by
 * log2(e)/sqrt(d) (the kernel works in the exp2 domain). d in {64,128}; N % 128 == 0 (d=64) or % 64. */
int dfot_op_attention(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int heads, int n,
                      int d, int variant, void* stream);
/* same with a logical head dim d <= 128 (d % 4 == 0) stored in rows of dstride = (d <= 64 ? 64 : 128) elements whose
 * pad columns are zero; o[B,N,heads*d] is compact (row stride ldo) */
int dfot_op_attention_padded(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int heads, int n,
                             int d, void* stream);
/* dfot_op_attention_padded for sequences of exactly 64 tokens (the per-frame spatial attention of FacDiT / FacMatDiT at 64 patches per
 * frame): q, k, v [nseq][heads][64][dstride] bf16 with dstride = (d <= 64 ? 64 : 128), pad columns zero, q pre-scaled by log2(e)/sqrt(d);
 * o[(seq*64 + row)][head*d + c], c < d, compact with row stride ldo; only those columns are written.  One workgroup per (sequence,
 * head) with a single-pass softmax: the bits of a sequence depend on (d, its operands) alone, never on nseq or on the other sequences,
 * and no row outside the nseq sequences is read or written (the operand buffers need no slack).  d % 8 == 0, 0 < d <= 128, nseq > 0,
 * heads > 0, ldo % 8 == 0 covering heads*d; anything else: DFOT_ERR_SHAPE (null pointers: DFOT_ERR_ARG), nothing launched */
int dfot_op_attention_seq64(const void* q, const void* k, const void* v, void* o, int ldo, int nseq, int heads, int d, void* stream);
/* backward of dfot_op_attention_seq64 for the upstream gradient d_o[(seq*64 + row)][head*d + c] bf16 (row stride ldo; nothing beyond a
 * head's d columns is read) of o: dq, dk, dv in the layout of q, k, v (live columns c < d only; pad columns are not written).  One launch,
 * one workgroup per (sequence, head): scores, the single-pass softmax and delta are recomputed from q, k, v and d_o, so nothing but the
 * forward's operands is needed (no lse, no o).  dq is the gradient of the UNSCALED q (the factor 1/sqrt(d) is applied), dk carries
 * ln 2 (q holds log2 e).  The bits of a sequence depend on (d, its operands) alone, and no row outside the nseq sequences is read or
 * written.  The forward's shape rules: d % 8 == 0, 0 < d <= 128, nseq > 0, heads > 0, nseq*heads < 2^31, ldo % 8 == 0 covering heads*d;
 * anything else: DFOT_ERR_SHAPE (null pointers: DFOT_ERR_ARG), nothing launched */
int dfot_op_attention_seq64_bwd(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dq, void* dk, void* dv, int nseq,
                                int heads, int d, void* stream);
/* dfot_op_attention_seq64_bwd with its results stored straight into the packed gradient rows the QKV Linear's backward reads: row
 * seq*64 + r of dqkv (row stride ldg) holds dq of head hd at columns hd*d .. hd*d + d - 1, dk at heads*d + hd*d, dv at 2*heads*d + hd*d
 * -- bit for bit what dfot_op_dit_qkv_grad_pack (no rope table) makes of dfot_op_attention_seq64_bwd's three outputs, in one launch.
 * Columns at or beyond 3*heads*d and rows beyond nseq*64 are not written.  The shape rules of dfot_op_attention_seq64_bwd, and
 * ldg >= 3*heads*d with ldg % 8 == 0; anything else: DFOT_ERR_SHAPE (null pointers: DFOT_ERR_ARG), nothing launched */
int dfot_op_attention_seq64_bwd_packed(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dqkv, int ldg, int nseq,
                                       int heads, int d, void* stream);
/* temporal attention of the factorized-attention DiT: q, k, v [batch*tokens][heads][patches][dstride] bf16 as above (what the per-frame
 * QKV epilogue writes; q pre-scaled); for every (video, head, patch position) the `tokens` frames of the video attend to each other.
 * o[(video, frame, patch)][heads*d] compact (row stride ldo).  1 <= tokens <= 32, d % 4 == 0, d <= 128, patches % 128 == 0, ldo a
 * multiple of 8 (4 when d % 8 != 0) covering heads*d; anything else: DFOT_ERR_SHAPE */
int dfot_op_attention_temporal(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int tokens, int patches,
                               int heads, int d, void* stream);
/* backward of dfot_op_attention_temporal for the upstream gradient d_o [(video, frame, patch)][heads*d] bf16 (row stride ldo) of o: dq,
 * dk, dv in the layout of q, k, v (live columns only; pad columns are not written).  Scores, softmax (with the forward's bf16-rounded
 * probabilities), dP and dS are recomputed: no log-sum-exp, no delta buffer.  dq is the gradient of the UNSCALED q (factor 1/sqrt(d)) and
 * dk carries ln 2, as dfot_op_attention_bwd.  Fixed summation order, no atomics: a video gives the same bits alone, in a batch and on
 * repeat.  1 <= tokens <= 32, d % 8 == 0, d <= 128, patches % 128 == 0, ldo a multiple of 8 covering heads*d, batch and heads <= 65535;
 * anything else: DFOT_ERR_SHAPE (null pointer: DFOT_ERR_ARG) before any launch, nothing written */
int dfot_op_attention_temporal_bwd(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dq, void* dk, void* dv,
                                   int batch, int tokens, int patches, int heads, int d, void* stream);
/* dfot_op_attention_temporal_bwd at 64 patches per frame, the shape the FacDiT trainer runs the kernel at for the res-128 recipes (the
 * op above keeps refusing it).  Every other rule is that op's; any 1 <= tokens <= 32 */
int dfot_op_attention_temporal_bwd_p64(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dq, void* dk, void* dv,
                                       int batch, int tokens, int heads, int d, void* stream);
/* MatrixAttention core of the FacMatDiT backbone (DiT3D "factorized_matrix_attention", engine variant 3): every frame is one token whose
 * q / k / v are (E/cc x h/rr) matrices.  z [batch*L*E][3h] bf16 holds (q|k|v), rows (frame, col head, n), columns (row head, d);
 * o [batch*L*E][h] in the same order.  Per (video, col head, row head): S[l][l'] = scale * <rope(q_l), rope(k_l')> over the matrix
 * entries, softmax over l', o = P v.  rope_cs: fp32 [rows >= L][h/rr/2][2] = (cos, sin) of frame l and pair i, applied to the
 * interleaved pairs (d = 2i, 2i + 1) of every matrix row; NULL = no rotation.  Every q, k, v entry is read once for every L.
 * 1 <= L <= 32, E % cc == 0, h % rr == 0, (h/rr) % 4 == 0; anything else: DFOT_ERR_SHAPE before any launch */
int dfot_op_matrix_attention_rope(const void* z, void* o, const float* rope_cs, int batch, int L, int E, int h, int cc, int rr,
                                  float scale, void* stream);
/* backward of dfot_op_matrix_attention_rope: dz [batch*L*E][3h] bf16 (dq|dk|dv) for the upstream gradient d_o [batch*L*E][h] bf16 of o, in
 * the forward's layouts.  q and k are rotated as the forward rotates them (S is the forward's S) and dq / dk are rotated back with the
 * angle of their own frame.  Fixed summation order, no atomics: a video gives the same bits alone, in a batch and on repeat.  Same shape
 * rules and error codes as the forward, checked before any launch; dz must not alias z or d_o (DFOT_ERR_ARG); rope_cs NULL = no rotation */
int dfot_op_matrix_attention_rope_bwd(const void* z, const void* d_o, const float* rope_cs, void* dz, int batch, int L, int E, int h, int cc,
                                      int rr, float scale, void* stream);
/* Gradient of a left factor (qkv_u, proj_u) of the MatrixDiTBlock at 64 patches per frame, operands as the training step leaves them:
 *   out[ra][rb] (fp32) = sum_f sum_d a[f][ra][d] * b[f][rb][d],   a [frames][Ra][hd], b [frames][Rb][hd] bf16, no copies, no padding.
 * dU'[e][p] is (a = o, b = ds), dU[p][e] is (a = m, b = dw1).  bf16 MFMA with fp32 accumulation; the frame axis is split over workgroups,
 * every slice stores its partial tile to a workspace of the library's own and one pass sums the slices in slice order: no atomics, the
 * same bits on every call.  Ra, Rb in {64, 128}, hd % 128 == 0, frames >= 1 (anything else: DFOT_ERR_SHAPE); a null a, b or out:
 * DFOT_ERR_ARG; both before any launch.  Test / measurement entry of the launcher the engine calls */
int dfot_op_facmat_factor_wgrad(const void* a, const void* b, float* out, int frames, int ra, int rb, int hd, void* stream);
/* the DifferenceDiT3D (variant 1) form of the same core, without rotation: register forms for L in {2, 4, 6, 8, 10}, one pair of
 * tokens per wave pass for every other L <= 32.  Test / measurement entry of the engine's own launcher */
int dfot_op_matrix_attention(const void* z, void* o, int batch, int L, int E, int h, int cc, int rr, float scale, void* stream);
/* Left factors of the MatrixDiTBlock at narrow column widths, 1 <= E <= 32 (FacMatDiT S-1-1 .. S-32-4, B-1-1 .. B-32-1), in the natural
 * layouts -- no per-frame transpose before or after.  All operands bf16, sums fp32, outputs rounded to bf16.
 *   contract: w[f][e][d] = sum_p u[e][p] * m[f][p][d]   m [frames][P][h] (the modulated frame), u [E][P] (qkv_u transposed), w [frames][E][h]
 *   expand:   s[f][p][d] = sum_e u[p][e] * o[f][e][d]   o [frames][E][h] (the attention output), u [P][E] (proj_u transposed), s [frames][P][h]
 * Streaming kernels: one wave owns 64 columns of one frame (expand: and 32 rows); a frame's sums are formed in an order fixed by (P, E)
 * alone -- no atomics, the same bits for a frame alone and inside any batch -- and nothing outside the stated extents is read or written.
 * frames >= 1, 1 <= E <= 32 (odd widths included), P % 64 == 0, h % 64 == 0, h <= 2048, 16-byte aligned pointers; anything else:
 * DFOT_ERR_SHAPE (null / misaligned pointer: DFOT_ERR_ARG) with the op named in dfot_last_error(), before any device work */
int dfot_op_facmat_contract(const void* m, const void* u, void* w, int frames, int P, int h, int E, void* stream);
int dfot_op_facmat_expand(const void* o, const void* u, void* s, int frames, int P, int h, int E, void* stream);
/* Attention-map kernels (test / measurement entries; see the dfot_dit_capture_attention section).  All outputs fp32; fixed summation order, no
 * atomics: two calls give the same bits.  None of them writes q, k or z.
 * Full attention: q, k as dfot_op_attention_padded takes them, n = tokens * patches with n % 128 == 0, patches % 64 == 0, 1 <= tokens <= 32.
 * form DFOT_ATTN_MAP_FULL: out [batch][heads][n][n]; DFOT_ATTN_MAP_FRAME: out [batch][heads][tokens][tokens], and `workspace` holds at least
 * the bytes the query below returns (temporal = 0).  Anything else: DFOT_ERR_SHAPE before any device work */
size_t dfot_op_attention_map_workspace_bytes(int temporal, int batch, int heads, int tokens, int patches);
int dfot_op_attention_map(const void* q, const void* k, void* out, void* workspace, size_t workspace_bytes, int form, int batch, int heads,
                          int n, int tokens, int d, void* stream);
/* Temporal attention: q, k as dfot_op_attention_temporal takes them; out [batch][heads][tokens][tokens] = the mean over the patch positions of
 * the T x T softmax of every (video, head, patch).  patches % 64 == 0, 1 <= tokens <= 32, d % 4 == 0, d <= 128; workspace: the query with
 * temporal = 1 */
int dfot_op_attention_temporal_map(const void* q, const void* k, void* out, void* workspace, size_t workspace_bytes, int batch, int tokens,
                                   int patches, int heads, int d, void* stream);
/* Matrix attention: z, rope_cs (NULL = no rotation), scale and the shape rules of dfot_op_matrix_attention_rope; out [batch][cc][rr][L][L] */
int dfot_op_matrix_attention_map(const void* z, const float* rope_cs, void* out, int batch, int L, int E, int h, int cc, int rr, float scale,
                                 void* stream);
/* training path, test entry: o = attention(q, k, v) as above and, for the upstream gradient d_o [B*N][ldo] (same compact layout as
 * o), dq / dk / dv in the layout of q / k / v; dq is the gradient of the UNSCALED q (q itself is passed pre-multiplied by
 * log2(e)/sqrt(d), as the forward wants it).  Replaces torch autograd through F.scaled_dot_product_attention
 * (algorithms/dfot/backbones/dit/dit_blocks.py:21-44,100-123). */
int dfot_op_attention_bwd(const void* q, const void* k, const void* v, const void* d_o, void* o, int ldo, void* dq, void* dk, void* dv,
                          int batch, int heads, int n, int d, void* stream);
/* training path of the UViT3DPose ResBlocks / resamplers, test entry: gradients of y = conv3x3(x, w, padding 1) + b for the upstream
 * gradient dy: x [BT,H,W,Cin] and dy [BT,H,W,Cout] bf16 channels-last, w fp32 [Cout][Cin][3][3]; dx fp32 [BT,H,W,Cin], dw fp32 like w,
 * db fp32 [Cout].  Channel counts multiples of 64, BT*H*W a multiple of 128 (the data-gradient GEMM takes whole 128-row tiles); anything
 * else returns DFOT_ERR_SHAPE before a byte is written.  Replaces autograd through F.conv2d (u_vit_blocks.py:16-93). */
int dfot_op_conv3x3_bwd(const void* x, const void* dy, const float* w, float* dx, float* dw, float* db, int bt, int h, int w_, int cin, int cout,
                        void* stream);
/* the same (shape rules included: channels % 64 == 0, BT*H*W % 128 == 0, DFOT_ERR_SHAPE before a byte is written) with the data gradient in
 * fp32 (dx) OR in bf16 (dx_bf; exactly one of the two, anything else DFOT_ERR_ARG): a gradient that only feeds the backward of the
 * GroupNorm in front of the convolution is written once, at half the bytes -- what torch.autocast(bf16) leaves there in the reference
 * (F.conv2d runs in bf16 under the trainer's precision setting, configurations/experiment/base_pytorch_exp.yaml:12 `precision: bf16`). */
int dfot_op_conv3x3_bwd2(const void* x, const void* dy, const float* w, float* dx, void* dx_bf, float* dw, float* db, int bt, int h, int w_, int cin,
                         int cout, void* stream);
/* test entry: backward of y = SiLU(FiLM(GroupNorm32(x))) (ResBlock in_layers: film NULL; out_norm: film [BT*P][2C] bf16 = scale | shift,
 * u_vit_blocks.py:57-93): x, dy, dx fp32 [BT][P][C]; dfilm bf16 like film; dgamma / dbeta fp32 [C] */
int dfot_op_gn_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const void* film, float eps, float* dx, void* dfilm,
                        float* dgamma, float* dbeta, int bt, int pixels, int channels, void* stream);
/* test entries of the UViT TransformerBlock backward pieces (u_vit_blocks.py:96-116,192-281):
 * NormalizeWithCond: xn = RMSNorm(x; w) (1 + scale) + shift with film [rows][2C] bf16 = (scale | shift): dx fp32, dfilm bf16, dw fp32 [C] */
int dfot_op_rms_film_bwd(const float* x, const float* dxn, const float* w, const void* film, float eps, float* dx, void* dfilm, float* dw,
                         int64_t rows, int channels, int accumulate_dx, void* stream);
/* the same out of place: dx = dres + the norm's input gradient (dres is the gradient of the residual path, left untouched);
 * dx_bf (optional, bf16 [rows][channels]): a bf16 copy of dx, the GEMM operand of the block below */
int dfot_op_rms_film_bwd_res(const float* x, const float* dxn, const float* w, const void* film, float eps, const float* dres, float* dx, void* dx_bf,
                             void* dfilm, float* dw, int64_t rows, int channels, void* stream);
/* per-head q / k RMSNorm + RoPE (rope_cs [ntok][d/2][2] = cos, sin): fused [rows][ld] bf16 holds (q | k | v) head-major in its first 3C
 * columns, dq / dk / dv [B][heads][ntok][d] bf16 are the attention backward's outputs; writes dfused [rows][ldo] columns [0, 3C), dqw / dkw [d] */
int dfot_op_qknorm_rope_bwd(const void* fused, int ld, const void* dq, const void* dk, const void* dv, const float* qw, const float* kw,
                            const float* rope_cs, float eps, void* dfused, int ldo, float* dqw, float* dkw, int64_t rows, int ntok, int heads, int d,
                            void* stream);
/* token-axis weight-gradient GEMM: out [M][N] fp32 = a^T b, a [rows][lda] and b [rows][ldb] bf16 in the activations' own
 * (feature-contiguous) layout (either may be a column block of a wider matrix); M, N multiples of 8, rows of 64.
 * slices == 0: tile form (128x128 / 256x256 / 256x192 / 192x256, LDS-DMA staged) and K slices chosen by shape (wgrad_plan);
 * slices >= 1: the 128x128 form with that many K slices.  Partial buffers are summed inside. */
int dfot_op_wgrad_nt(const void* a, int lda, const void* b, int ldb, float* out, int m, int n, int64_t rows, int slices, void* stream);
/* op-level entry points a training driver composes (all on device pointers, bf16 activations unless noted):
 * out = a w^T (+ bias) in bf16 / fp32 (+ resid); transposes; column sums; the training-form forwards of the UViT TransformerBlock pieces
 * (values the backward needs are kept: no fused norm / activation epilogues); attention with its log-sum-exp and the backward from it */
int dfot_op_gemm_bf16(const void* a, int lda, const void* w, const float* bias, void* out, int ldo, int m, int n, int k, void* stream);
int dfot_op_gemm_f32(const void* a, int lda, const void* w, const float* bias, const float* resid, float* out, int ldo, int m, int n, int k,
                     void* stream);
int dfot_op_transpose_bf16(const void* src, void* dst, int rows, int cols, void* stream);
int dfot_op_colsum_bf16(const void* src, int ld, float* out, int64_t rows, int n, void* stream);
int dfot_op_rms_film_fwd(const float* x, const float* w, const void* film, float eps, void* out, int64_t rows, int channels, void* stream);
/* fused_attn_mlp_proj of a TransformerBlock in its training form, one launch (u_vit_blocks.py:253-262): the raw projection (bias added) is kept
 * as bf16 `fused` [rows][7C] for the backward, and the same epilogue writes q, k (per-head RMSNorm + RoPE; q * qscale), v as
 * [B][heads][ntok][d] and SiLU(mlp_h) into cat[:, ccol0 : ccol0 + 4C] (row stride ldcat) */
int dfot_op_fused_proj_train(const void* a, int lda, const void* w, const float* bias, const float* qw, const float* kw, const float* rope_cs, float eps,
                             float qscale, void* fused, void* q, void* k, void* v, void* cat, int ldcat, int ccol0, int64_t rows, int ntok, int heads,
                             int d, void* stream);
int dfot_op_qknorm_rope_fwd(const void* fused, int ld, const float* qw, const float* kw, const float* rope_cs, float eps, float qscale, void* q,
                            void* k, void* v, int64_t rows, int ntok, int heads, int d, void* stream);
int dfot_op_silu_cols(const void* src, int lds_, int scol0, const void* grad, int ldg, int gcol0, void* dst, int ldd, int dcol0, int64_t rows,
                      int ncols, void* stream);
/* the same with a caller-supplied bound of the scores in the log2 domain (< 64: the d = 64 launch may run without a running max; anything
 * else, NaN included, takes the running-max kernel).  scratch: device buffer of at least dfot_op_attention_scratch_bytes(...) bytes for the
 * fp32 partial rows of the key-split tail, owned by the caller (one per trainer / stream); null = a process-wide grow-only block */
size_t dfot_op_attention_scratch_bytes(int batch, int heads, int n, int d);
int dfot_op_attention_fwd_lse_bounded(const void* q, const void* k, const void* v, void* o, int ldo, float* lse, int batch, int heads, int n, int d,
                                      float score_bound, void* scratch, size_t scratch_bytes, void* stream);
int dfot_op_attention_fwd_lse(const void* q, const void* k, const void* v, void* o, int ldo, float* lse, int batch, int heads, int n, int d,
                              void* stream);
int dfot_op_attention_bwd_lse(const void* q, const void* k, const void* v, const void* o, const void* d_o, int ldo, const float* lse, float* delta,
                              void* dq, void* dk, void* dv, int batch, int heads, int n, int d, void* stream);
/* ResBlock / resampler / embedding pieces of the UViT training driver (channels-last fp32 streams, bf16 GEMM operands).
 * Shape contract of the vectorised kernels: GroupNorm entries take 128, 256, 512 or 1024 channels; pool2_bf16 / pool2_bwd / upsample_add /
 * upsample_bwd channels % 4 == 0 and, except upsample_add (which takes the coarse size), even h and w; frame sums / split_bf16 lengths
 * % 8 == 0, split_bf16 pointers 16-byte aligned; cond_repack kpad >= 4 cdim (anything else returns DFOT_ERR_SHAPE or DFOT_ERR_ARG). */
int dfot_op_gn_silu_fwd(const float* x, const float* gamma, const float* beta, const void* film, float eps, void* out, float* stats, int bt,
                        int pixels, int channels, void* stream);


/* backward of GroupNorm (+ FiLM) + SiLU with saved statistics, the upstream gradient dy in bf16 [BT][P][C] (dx_bf of dfot_op_conv3x3_bwd2):
 * dx = (dres ? dres : 0) + input gradient, as fp32 (dx) and / or bf16 (dx_bf); dfilm optional with its row stride dfilm_ld */
int dfot_op_gn_silu_bwd5(const float* x, const void* dy_bf, const float* stats, const float* gamma, const float* beta, const void* film, const float* dres,
                         float* dx, void* dx_bf, void* dfilm, int64_t dfilm_ld, float* dgamma, float* dbeta, int bt, int pixels, int channels,
                         void* stream);
/* Folded FiLM (training).  The reference computes emb = PatchEmbed(pose rays) keep + noise embedding per pixel (u_vit3d_pose.py:63-131,
 * embeddings.py:390-428), pools it down the levels and every block projects it: film = emb_layer(emb) (u_vit_blocks.py:57-116).  All of
 * these maps are linear, so film = (W_emb_layer W_patch) patches + [W_emb_layer (b_patch keep + noise_emb[frame]) + b]: the per-row part is a
 * GEMM over the 768-wide pose patches instead of the 1024-wide embedding, the per-frame part a [frames][2C] fp32 table added in that GEMM's
 * epilogue, and the backward never forms a per-row embedding gradient (uvit_train.py, UViT3DPoseTrainer.sync).
 * out bf16 [M][N] = a w^T + frame_bias[row / rows_per_frame][:] */
int dfot_op_gemm_bf16_frame_bias(const void* a, int lda, const void* w, const float* frame_bias, int rows_per_frame, void* out, int ldo, int m, int n, int k,
                                 void* stream);
/* GroupNorm + FiLM + SiLU with the block's (scale | shift) columns given as a column block of a level-wide matrix (row pitch film_ld >= 2C) */
int dfot_op_gn_silu_fwd2(const float* x, const float* gamma, const float* beta, const void* film, int64_t film_ld, float eps, void* out, float* stats,
                         int bt, int pixels, int channels, void* stream);
int dfot_op_gn_silu_bwd6(const float* x, const void* dy_bf, const float* stats, const float* gamma, const float* beta, const void* film,
                         int64_t film_ld, const float* dres, float* dx, void* dx_bf, void* dfilm, int64_t dfilm_ld, float* dgamma, float* dbeta, int bt,
                         int pixels, int channels, void* stream);
/* Per-frame FiLM forms of the four training norm ops (pose-free UViT3D: the conditioning embedding is one vector per frame, u_vit3d.py:306-310).
 * film_vec fp32 [frames][film_ld] holds the block's (scale | shift) in columns 0..C | C..2C and may be a column block of a level-wide table
 * (film_ld >= 2C, a multiple of 4 floats; the pointer 16-byte aligned).  The backward writes the FiLM gradient already summed over each frame's
 * rows, dfilm_vec fp32 [frames][dfilm_ld]: dscale[f][c] = sum_rows dz (xhat gamma + beta) | dshift[f][c] = sum_rows dz -- fixed-order fp32 sums of
 * per-workgroup partial rows (no atomics: bit-reproducible), no [rows][2C] tensor read or written.  dgamma / dbeta / dw are written, not
 * accumulated.  Shapes: channels 128, 256, 512 or 1024 (GroupNorm), a width with a LayerNorm kernel instance (RMS: 64 k, k odd <= 9, or 128 k,
 * k <= 10, 12, 16), rows a multiple of rows_per_frame; anything else returns DFOT_ERR_SHAPE or DFOT_ERR_ARG before any launch. */
int dfot_op_gn_silu_fwd_frame(const float* x, const float* gamma, const float* beta, const float* film_vec, int64_t film_ld, float eps, void* out,
                              float* stats, int bt, int pixels, int channels, void* stream);
int dfot_op_gn_silu_bwd_frame(const float* x, const void* dy_bf, const float* stats, const float* gamma, const float* beta, const float* film_vec,
                              int64_t film_ld, const float* dres, float* dx, void* dx_bf, float* dfilm_vec, int64_t dfilm_ld, float* dgamma,
                              float* dbeta, int bt, int pixels, int channels, void* stream);
int dfot_op_rms_film_fwd_frame(const float* x, const float* w, const float* film_vec, int64_t film_ld, float eps, void* out, int64_t rows,
                               int64_t rows_per_frame, int channels, void* stream);
int dfot_op_rms_film_bwd_frame(const float* x, const float* dxn, const float* w, const float* film_vec, int64_t film_ld, float eps, const float* dres,
                               float* dx, void* dx_bf, float* dfilm_vec, int64_t dfilm_ld, float* dw, int64_t rows, int64_t rows_per_frame, int channels,
                               void* stream);
/* out [bt][n] fp32 = per-frame column sums of src bf16 [bt * pixels][ld] (the gradient of the per-frame FiLM table from the FiLM gradients) */
int dfot_op_frame_sums_bf16(const void* src, int64_t ld, float* out, int bt, int pixels, int n, void* stream);
/* x fp32 = hi + lo, both bf16 (lo carries the next 8 mantissa bits): three bf16 products Ah Bh + Ah Bl + Al Bh with fp32 accumulation
 * reproduce an fp32 product to ~2^-16 -- how the weight-sized products of the folded FiLM run on the matrix cores */
int dfot_op_split_bf16(const float* x, void* hi, void* lo, int64_t n, void* stream);
/* C[i][j] (+)= sum_k A[i * sa_i + k * sa_k] * B[k * sb_k + j * sb_j] in fp32 with element strides: the weight-sized products of the
 * folded FiLM (W_emb_layer W_patch and the gradients back to the two factors) */
int dfot_op_sgemm(const float* a, int64_t sa_i, int64_t sa_k, const float* b, int64_t sb_k, int64_t sb_j, float* c, int64_t ldc, int m, int n, int k,
                  int accumulate, void* stream);
int dfot_op_pack_conv3(const float* w, void* out, int co, int ci, int dgrad, void* stream);
int dfot_op_conv3x3_f32(const void* a, const void* w, const float* bias, const float* resid, float* y, int bt, int h, int w_, int cin, int cout,
                        void* stream);
int dfot_op_pool2_bf16(const float* x, void* out, int bt, int h, int w, int c, void* stream);
int dfot_op_pool2_bwd(const float* dp, float* dx, int bt, int h, int w, int c, void* stream);
int dfot_op_sub_bf16(const float* a, const float* b, void* out, int64_t n, void* stream);
int dfot_op_upsample_add(const float* t, const float* skip, float* out, int bt, int h, int w, int c, void* stream);
int dfot_op_upsample_bwd(const float* dy, float* ds, int bt, int h, int w, int c, void* stream);
int dfot_op_axpy(float* a, const float* b, float alpha, int64_t n, void* stream);
int dfot_op_mul_cols(void* dst, int ldd, int dcol0, const void* mask, int64_t rows, int ncols, void* stream);
int dfot_op_emb_pyramid(const void* emb0, void* emb1, void* emb2, void* emb3, int bt, int r0, int e, void* stream);
int dfot_op_cond_repack(const float* cond, void* a, int bt, int res, int cdim, int kpad, void* stream);
int dfot_op_embed_input(const float* x, const float* w, const float* b, float* out, int bt, int res, int cin, int c0, void* stream);
int dfot_op_embed_input_wgrad(const float* dx0, const float* x, float* dw, float* db, int bt, int res, int cin, int c0, int ps, void* stream);
/* gradient w.r.t. the backbone input x [BT][Cin][R][R] of the patch embedding (dx0 fp32 [pix][C0], w [C0][Cin][2][2]): the last step of
 * d prediction / d x_t, which reconstruction guidance needs (discrete_diffusion.py:485-513) */
int dfot_op_embed_input_dgrad(const float* dx0, const float* w, float* dx, int bt, int res, int cin, int c0, int ps, void* stream);
int dfot_op_project_output(const float* x0, const float* w, const float* b, float* out, int bt, int res, int c0, int cout, void* stream);
int dfot_op_outgrad_gather(const float* dout, void* dpatch, int bt, int res, int cout, int ps, void* stream);
/* fp32 <-> bf16 helpers for tests */
int dfot_op_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int dfot_op_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
/* exact comparison of two device buffers of `bytes` bytes: *differs (device int32, 4-byte aligned, zeroed by the caller on the same stream)
 * is set to 1 when any BIT differs -- equal NaN payloads compare equal, +0.0 and -0.0 do not -- and is left untouched otherwise, so several
 * calls may share one flag.  Reads 2 x bytes in 16-byte loads when both bases are 16-byte aligned (scalar loads otherwise, and for the
 * tail), writes at most 4 bytes; no atomics.  bytes == 0: equal, nothing is launched.  Null or misaligned flag, null buffer with
 * bytes > 0, bytes < 0: DFOT_ERR_ARG before any launch.  The content key of the UViT3DPose pose / FiLM cache (backbone.py). */
int dfot_op_equal_bits(const void* a, const void* b, int64_t bytes, int32_t* differs, void* stream);

/* ---- VideoVAE decoder pieces (algorithms/vae/video_vae/model.py:130-281, algorithms/vae/common/modules/{conv,resnet,attention,
 * updownsample,normalize}.py; called from BaseVideoAlgo._decode, algorithms/common/base_pytorch_video_algo.py:600-629).  Channels-last
 * activations [B][T][H][W][C]; the 3x3(x3) convolutions and 1x1x1 projections go through dfot_op_conv3x3_f32 / dfot_op_gemm_*. ------- */
/* GroupNorm(32 groups, eps) over the `pixels` (= T*H*W of one video) positions of each of the bt items, then optional SiLU: fp32 -> bf16.
 * scratch: dfot_op_groupnorm_scratch_floats(bt, pixels) floats.  channels in {128, 256, 512, 1024}. */
int64_t dfot_op_groupnorm_scratch_floats(int bt, int pixels);
int dfot_op_groupnorm(const float* x, const float* gamma, const float* beta, float eps, void* out, float* scratch, int bt, int pixels,
                      int channels, int silu, void* stream);
/* out[b][t] = x[b][max(t - shift, 0)] (bf16, frame_elems per frame): the first-frame-replicating causal pad of PaddedConv3D (conv.py:104-109) */
int dfot_op_frame_shift(const void* x, void* out, int batch, int frames, int64_t frame_elems, int shift, void* stream);
/* fp32 [B][T][H][W][C] -> [B][T'][2H][2W][C]; mode 0: nearest in (H, W), T' = T (SpatialUpsample2x, updownsample.py:77-83); mode 1: the
 * causal trilinear upsample of Spatial2xTime2x3DUpsample (:143-150), T' = 1 + 2 (T - 1) */
int dfot_op_upsample3d(const float* x, float* out, int batch, int frames, int h, int w, int channels, int mode, void* stream);
/* probs[r][:] = softmax(scale * scores[r][:]) (fp32 -> bf16): the frame-wise single-head attention of AttnBlock3D (attention.py:127-129) */
int dfot_op_softmax_rows(const float* scores, void* probs, int64_t rows, int n, float scale, void* stream);
/* ---- VideoVAE encoder pieces (algorithms/vae/video_vae/model.py:38-150,402-443, updownsample.py Downsample /
 * Spatial2xTime2x3DDownsample, distribution.py; called from BaseVideoAlgo._encode, base_pytorch_video_algo.py:585-596). ------------------- */
/* y fp32 [B][To][H][W][Cout] (+ bias, + resid fp32 of the same shape) = convolution of a bf16 [B][Tin][Hin][Win][Cin] with w bf16
 * [Cout][kt][3][3][Cin] (K = kt*9*Cin tap-major), one launch.  Source frame of output frame t_o and temporal tap dt:
 * max(stride_t * t_o + dt - (kt - 1), 0) (causal first-frame replication); source pixel (s y_o + dy - p, s x_o + dx - p), p = 1 for s = 1
 * and 0 for s = 2 (zero padding (0, 1)).  H = Hin / s, W = Win / s, To = (Tin - 1) / stride_t + 1.  kt in {1, 3}, s and stride_t in
 * {1, 2}, Cin % 64 == 0, Cout % 4 == 0, B*To*H*W a multiple of 128. */
int dfot_op_conv3t_f32(const void* a, const void* w, const float* bias, const float* resid, float* y, int batch, int t_in, int h_in, int w_in,
                       int cin, int cout, int kt, int stride_s, int stride_t, void* stream);
/* out bf16 [B][T][H][W][64] = a * x + b on channels 0-2, 0 on 3-63; x fp32 (B, 3, T, H, W) addressed with element strides sb, sc, st, sh, sw
 * (any permutation of the layout) */
int dfot_op_vae_pixels(const float* x, int64_t sb, int64_t sc, int64_t st, int64_t sh, int64_t sw, float a, float b, void* out, int batch, int frames,
                       int h, int w, void* stream);
/* DiagonalGaussianDistribution of the moments fp32 [B][T][hw][ld] (mean = channels [0, zc), logvar = [zc, 2 zc) clamped to [-30, 20]), every
 * output fp32 [B][T][zc][hw] (b t c h w) and optional: mean, logvar, std = exp(logvar / 2), z = mean + std * eps (eps in the same layout;
 * NULL: z = mean), then z = (z - data_mean[c]) / data_std[c] when both are given. */
int dfot_op_vae_posterior(const float* moments, int ld, const float* eps, const float* data_mean, const float* data_std, float* mean, float* logvar,
                          float* std_, float* z, int batch, int frames, int hw, int zc, void* stream);

/* ---- ImageVAE pieces (algorithms/vae/image_vae/model.py:18-245; AttnBlock attention.py:39-83, Upsample / Downsample
 * updownsample.py:10-45): per-frame layers on channels-last [frames][H][W][C] activations. ------------------------------------------- */
/* o bf16 [frames*n][c] = softmax(q k^T / sqrt(c)) v per frame: ONE head over the n positions of a frame with all c channels, every frame in
 * one launch, no score matrix in memory (fp32 softmax with the row max subtracted, P rounded to bf16).  q, k, v bf16 [frames*n][c].
 * n in {64, 256} (all scores of a row in registers) or a multiple of 256 in [512, 4096] (keys streamed in blocks of 128 with a running
 * max and sum: 1024 = a 256 x 256 frame at f8, 4096 = a 512 x 512 one), c a multiple of 128 up to 1024; other shapes: DFOT_ERR_SHAPE
 * before any device work.  One fixed summation order per (n, c): a frame's bits do not depend on the launch it is part of. */
int dfot_op_ivae_attention(const void* q, const void* k, const void* v, void* o, int frames, int n, int c, void* stream);
/* y fp32 [frames][h_in/2][w_in/2][cout] (+ bias) = Conv2d(k 3, s 2, p 0) of F.pad(x, (0, 1, 0, 1)): zero padding on the right and bottom only.
 * x bf16 [frames][h_in][w_in][cin], w bf16 [cout][9][cin] (dfot_op_pack_conv3).  h_in, w_in even, cin % 64 == 0, cout % 128 == 0. */
int dfot_op_conv3x3_s2_f32(const void* x, const void* w, const float* bias, float* y, int frames, int h_in, int w_in, int cin, int cout,
                           void* stream);
/* y fp32 [frames][2 h_in][2 w_in][cout] (+ bias) = Conv2d(k 3, s 1, p 1) of the nearest-2x upsampled x, the upsampling fused into the
 * gather (source pixel ((y + dy - 1) >> 1, (x + dx - 1) >> 1)).  Operands as dfot_op_conv3x3_s2_f32. */
int dfot_op_upconv3x3_f32(const void* x, const void* w, const float* bias, float* y, int frames, int h_in, int w_in, int cin, int cout,
                          void* stream);

/* ---- TiTok-KL decoder pieces (algorithms/vae/tiktok_kl/{titok_kl,blocks_kl}.py: the ViT over [cls | grid^2 mask tokens | latent tokens];
 * its GEMMs, the channel softmax and the pixel decoder are the ops above). ------------------------------------------------------------ */
/* The core of nn.MultiheadAttention on the packed in-projection output, for ragged sequences.  qkv bf16 [rows][ld]: columns q | k | v, each
 * heads adjacent groups of 64 channels (ld >= 3 * heads * 64, a multiple of 8); `seqs` sequences of `len` rows back to back (sequence s owns
 * rows s * len .. s * len + len - 1); o bf16 [rows][heads * 64] = softmax(q k^T / 8) v per sequence and head.  Any 1 <= len <= the value of
 * the max_len query (4160), 1 <= heads <= 64; anything else: DFOT_ERR_SHAPE before any device work.  The log2(e) / 8 scale is applied inside
 * the kernel (exp2 domain, fp32 softmax with the row max subtracted, P rounded to bf16).  Keys past len are masked by select; rows the
 * sequence does not own (another sequence's, the rows that pad `rows` to a GEMM tile) are never loaded for it, and rows of o outside the
 * seqs * len owned ones are not written.  One fixed summation order per (len, heads): a sequence's bits do not depend on seqs. */
int dfot_op_mha_packed(const void* qkv, int64_t ld, void* o, int seqs, int len, int heads, void* stream);
int dfot_op_mha_packed_max_len(void);
/* nn.LayerNorm (affine) of fp32 rows [rows][channels], channels in {512, 768, 1024}: out_bf16 and / or out_f32 (either may be NULL, not
 * both; out_f32 may be x itself in the plain form).  seq_len == 0: row r reads x row r (first = take = 0).  Gather form, seq_len > 0: output
 * row r reads x row (r / take) * seq_len + first + r % take, rows a multiple of take, first + take <= seq_len. */
int dfot_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, void* out_bf16, float* out_f32, int64_t rows, int channels,
                      int seq_len, int first, int take, void* stream);
/* out bf16 [rows][n] = act(x[rows][ld] + bias[n]); act 0 = GELU in the exact erf form (nn.GELU()), 1 = tanh.  n, ld multiples of 4. */
int dfot_op_bias_act_bf16(const float* x, int64_t ld, const float* bias, void* out, int64_t rows, int n, int act, void* stream);
/* The decoder's token sequence in one launch (blocks_kl.py:219-234): out fp32 [frames * (1 + grid2 + num_latent)][channels] = ln_pre of
 * [cls + pos[0] | mask_token + pos[1 .. grid2] | decoder_embed(z_n[:, t]) + latent_pos[t]], z fp32 (frames, token_size, 1, num_latent),
 * z_n = F.normalize(z, dim=1) when l2norm (x / max(|x|, 1e-12)), embed_w [channels][token_size].  token_size <= 64. */
int dfot_op_titok_tokens(const float* z, const float* embed_w, const float* embed_b, const float* latent_pos, const float* cls, const float* mask_token,
                         const float* pos, const float* gamma, const float* beta, float eps, float* out, int frames, int grid2, int num_latent,
                         int token_size, int channels, int l2norm, void* stream);

/* ---- TiTok-KL encoder pieces (blocks_kl.py:95-166; the ResidualAttentionBlocks, ln_post and the posterior are the ops above). ---------- */
/* The A operand of the patch-embedding GEMM (Conv2d(3, C, k 16, s 16)): rows bf16 [nframes * g^2][768], g = image_size / 16, from frames
 * fp32 (nframes, 3, image_size, image_size) contiguous:
 *   rows[f * g^2 + py * g + px][c * 256 + dy * 16 + dx] = bf16(frames[f][c][16 py + dy][16 px + dx])   (round to nearest even)
 * the flattening order of patch_embed.weight (C, 3, 16, 16).  Rows past nframes * g^2 are not written.  image_size a positive multiple of
 * 16; anything else: DFOT_ERR_SHAPE before any device work. */
int dfot_op_titok_patch_rows(const float* frames, void* rows_bf16, int nframes, int image_size, void* stream);
/* The encoder's token sequence in one launch (blocks_kl.py:140-154): out fp32 [frames * (1 + grid2 + num_latent)][channels] = ln_pre of
 * [cls + pos[0] | patches[f * grid2 + p] + pos[1 + p] | latent_tokens[t] + latent_pos[t]]; patches fp32 [frames * grid2][ldp] is the
 * patch-embedding GEMM's output with its bias (ldp >= channels, a multiple of 4).  channels in {512, 768, 1024}; fp32 statistics. */
int dfot_op_titok_enc_tokens(const float* patches, int64_t ldp, const float* cls, const float* pos, const float* latent_tokens, const float* latent_pos,
                             const float* gamma, const float* beta, float eps, float* out, int frames, int grid2, int num_latent, int channels,
                             void* stream);
/* conv_out (1x1, channels -> out_channels) on the reference's `reshape(batch, width, num_latent, 1)` of the contiguous ln_post rows
 * t fp32 [frames][num_latent][channels] (blocks_kl.py:163-165).  The reshape does not permute: it reads each frame's num_latent x channels
 * block as channels x num_latent, so
 *   out[f][n][o] = bias[o] + sum_c w[o][c] * t_f[c * num_latent + n]        (t_f the frame's block, flat)
 * w fp32 [out_channels][channels], out fp32 [frames][num_latent][ldo] (ldo >= out_channels): the moments layout dfot_op_vae_posterior
 * reads (batch = frames, frames = 1, hw = num_latent, zc = out_channels / 2).  All math fp32, one summation order per (num_latent, channels).
 * channels in {512, 768, 1024}, num_latent <= 128, out_channels even and <= 128; anything else: DFOT_ERR_SHAPE before any device work. */
int dfot_op_titok_moments(const float* t, const float* w, const float* bias, float* out, int64_t ldo, int frames, int num_latent, int channels,
                          int out_channels, void* stream);

/* ---- DC-AE pieces (algorithms/vae/dc_ae/autoencoder_dc_model.py:45-466: the deep-compression autoencoder of the dmlab / Minecraft latents;
 * its 3x3 and 1x1 convolutions are the ops above).  Channels-last operands, one launch for all frames, no atomics, no allocation; every
 * value depends on its own frame only, so a frame has the same bits alone and in any batch. -------------------------------------------- */
/* ReLU linear attention of SanaMultiscaleLinearAttention (:86-95) on the fused projection output qkv bf16 [frames * n][ld]: head g is the
 * 96 consecutive columns [96 g, 96 g + 96) = q | k | v of 32 channels each (the reference's reshape to (B, -1, 3 * 32, H W)).  Per frame
 * and head, in fp32:   S[j][d] = sum_n relu(k[n][j]) * [v[n] ; 1][d]   (32 x 33, positions summed in ascending order),
 *                      o[n][d] = (sum_j relu(q[n][j]) S[j][d]) / (sum_j relu(q[n][j]) S[j][32] + 1e-15),  d < 32
 * o bf16 [frames * n][heads * 32] (row stride ldo), head g at columns [32 g, 32 g + 32).  n a multiple of 64 in [64, 4096], heads in
 * [1, 64], ld >= 96 heads and ldo >= 32 heads, both multiples of 8; anything else: DFOT_ERR_SHAPE before any device work.  Rows past
 * frames * n are neither read nor written. */
int dfot_op_dcae_linear_attention(const void* qkv, int64_t ld, void* o, int64_t ldo, int frames, int n, int heads, void* stream);
/* The middle of GLUMBConv: depthwise Conv2d(2 hc, 2 hc, 3, 1, 1, groups = 2 hc) + bias on x bf16 [frames][h][w][2 hc], then
 * out[c] = y[c] * silu(y[hc + c]) as bf16 [frames][h][w][hc].  w_taps fp32 [9][2 hc] (tap dy * 3 + dx major, the transpose of the
 * reference's [2 hc][1][3][3]), bias fp32 [2 hc]; fp32 accumulation in tap order, pixels outside the map contribute nothing (zero padding).
 * hc a multiple of 256; x and out must not alias. */
int dfot_op_dcae_dw_glu(const void* x, const float* w_taps, const float* bias, void* out, int frames, int h, int w, int hc, void* stream);
/* DCDownBlock2d's tail (:226-240) and the encoder's output shortcut (:365-368), factor f in {1, 2}:
 *   out fp32 [frames][h / f][w / f][cout] = pixel_unshuffle(conv, f) + mean over groups of gs = f f cin / cout channels of pixel_unshuffle(src, f)
 * conv fp32 [frames][h][w][ldc] holds cout / f^2 channels (ldc >= that: the convolution's padded output), src fp32 [frames][h][w][cin]
 * (NULL: no shortcut).  Unshuffled channel e = c f^2 + dy f + dx is channel c of pixel (f Y + dy, f X + dx); the group is summed in
 * ascending order and divided by gs.  cout % 4 == 0, cout % f^2 == 0, f^2 cin % cout == 0. */
int dfot_op_dcae_down_shortcut(const float* conv, int64_t ldc, const float* src, float* out, int frames, int h, int w, int cin, int cout, int factor,
                               void* stream);
/* DCUpBlock2d's tail (:268-283) and the decoder's input shortcut (:453-455), factor f in {1, 2}:
 *   out fp32 [frames][f h][f w][cout] = pixel_shuffle(conv, f) + pixel_shuffle(repeat_interleave(src, rep), f),  rep = f f cout / cin
 * conv fp32 [frames][h][w][ldc] holds f^2 cout channels, src fp32 [frames][h][w][lds] holds cin (NULL: no shortcut).
 * f^2 cout % cin == 0. */
int dfot_op_dcae_up_shortcut(const float* conv, int64_t ldc, const float* src, int64_t lds, float* out, int frames, int h, int w, int cin, int cout,
                             int factor, void* stream);
/* Channel RMSNorm with weight and bias (diffusers RMSNorm(dim, eps, elementwise_affine, bias)) of fp32 rows [rows][channels]:
 *   y = x * rsqrt(mean(x^2) + eps) * weight + bias (+ resid) (relu: max(y, 0)),  written as fp32 and / or bf16 (either may be NULL, not both;
 * out_f32 may be x or resid).  fp32 statistics, one wave per row.  channels a multiple of 4 up to 2048. */
int dfot_op_dcae_rmsnorm(const float* x, const float* weight, const float* bias, float eps, const float* resid, float* out_f32, void* out_bf16,
                         int relu, int64_t rows, int channels, void* stream);
/* out bf16 [n] = act(x fp32 [n]); act 0 = none, 1 = ReLU, 2 = SiLU: a ResBlock's activation in front of conv2 (:129).  n % 4 == 0. */
int dfot_op_dcae_act_bf16(const float* x, void* out, int64_t n, int act, void* stream);

/* ---- DiT1D (algorithms/dfot/backbones/dit1d/dit_model.py:358-530 at the stock dit1d.yaml: merge_mode share_norm, no rotary embedding, no
 * qk-norm, no context tokens): the frame-causal transformer over 1-D token latents (B, T, C, 1, L), e.g. the [4, 1, 32] TiTok-KL frames. ---- */
/* Frame-causal ("block lower triangular") flash attention: operands and output exactly as dfot_op_attention_padded takes them (q, k, v
 * [B][heads][n][dstride] bf16 with dstride = (d <= 64 ? 64 : 128), pad columns zero, q pre-scaled by log2(e)/sqrt(d); o[(b*n + row)][head*d
 * + c], c < d, compact with row stride ldo, only those columns written).  n = frames * frame_len tokens; query i attends to key j iff
 * j / frame_len <= i / frame_len.  A workgroup owns 128 query rows and reads the keys below the end of its last frame only; masked
 * scores are replaced by -inf before the row maximum (never a bias), so they contribute exactly 0.  No atomics, no allocation, no host
 * synchronisation; the summation order depends on (n, frame_len, d) and the query tile alone: a video gives the same bits alone and in a
 * batch, and frames <= f give the same bits whatever frames > f hold (finite values).  frame_len in {16, 32, 64, 128}, n % 128 == 0,
 * d % 8 == 0, 0 < d <= 128, batch * heads * (n / 128) < 2^31 (the grid), ldo % 8 == 0 covering heads*d; anything else: DFOT_ERR_SHAPE (null pointers:
 * DFOT_ERR_ARG) before any device work. */
int dfot_op_attention_frame_causal(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int heads, int n, int frame_len,
                                   int d, void* stream);
/* The same forward for training: the same kernel body compiled with the log-sum-exp store, so o has the bits of
 * dfot_op_attention_frame_causal, and lse[(b*heads + head)*n + row] (fp32, must not be null: DFOT_ERR_ARG) receives the log2-domain
 * log-sum-exp m + log2(sum_j 2^(s_j - m)) of the row's visible scores.  Shape rules and refusals as above. */
int dfot_op_attention_frame_causal_lse(const void* q, const void* k, const void* v, void* o, int ldo, float* lse, int batch, int heads, int n,
                                       int frame_len, int d, void* stream);
/* Backward of the frame-causal attention under the contract of dfot_op_attention_bwd_lse: q, k, v as the forward read them, o / d_o compact
 * [(b*n + row)][ldo] (head hd at column hd*d; nothing beyond a head's d columns is read), lse from dfot_op_attention_frame_causal_lse,
 * delta [B][heads][n] fp32 scratch that receives sum_c d_o * o (computed here, then consumed), dq / dk / dv [B][heads][n][dstride] bf16
 * with the pad columns written as zero.  dq is the gradient of the UNSCALED q (it carries 1/sqrt(d)), dk carries the ln 2 that undoes
 * q's log2(e).  A workgroup owns 128 query rows (dq) or 128 key rows (dk/dv) and streams only the 64-row tiles on and below the block
 * diagonal; on the tiles that straddle it a masked score is selected to -inf before exp2 and its dS to 0 (a select on registers), so
 * large finite data in masked rows never reaches a sum.  No atomics, no split of a row across workgroups, no allocation after the first
 * call, no host synchronisation; the summation order depends on (n, frame_len, d) and the tile alone: a video gives the same bits alone
 * and in a batch, dq of frames <= f does not depend on frames > f, dk / dv of frames >= f do not depend on q / d_o of frames < f.
 * Shape rules of the forward (ldo is d_o's and o's row stride); null pointers: DFOT_ERR_ARG, shapes: DFOT_ERR_SHAPE, both before any
 * device work. */
int dfot_op_attention_frame_causal_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, int ldo, const float* lse,
                                       float* delta, void* dq, void* dk, void* dv, int batch, int heads, int n, int frame_len, int d,
                                       void* stream);

typedef struct dfot_dit1d_s* dfot_dit1d_t;
typedef struct {
  int32_t hidden;           /* hidden_size: a multiple of 64, <= 2048 */
  int32_t depth;
  int32_t heads;            /* head dim hidden / heads: a multiple of 8, <= 128 */
  int32_t mlp_hidden;       /* hidden * mlp_ratio: a multiple of 64 */
  int32_t in_channels;      /* C = x_shape[0], 1 .. 64 */
  int32_t tokens_per_frame; /* L = x_shape[2]: 16, 32, 64 or 128 */
  int32_t max_tokens;       /* T: frames per window; T * L a multiple of 128.  The model runs at exactly T frames (pos_embed fixes the length) */
  int32_t timesteps;        /* discrete noise levels 0 .. timesteps - 1 */
  int32_t causal;           /* 1: frame-causal attention (causal_attn_mode temporal_causal / video_temporal_causal); 0: no mask (null) */
  float eps;                /* LayerNorm epsilon (1e-6) */
} dfot_dit1d_config;
/* Parameters are enumerated in the reference module's state_dict order (pos_embed first: it is loaded, not recomputed) and loaded by name
 * as fp32 device tensors; dfot_dit1d_finalize tabulates the modulations of every noise level and synchronises.  dfot_dit1d_reserve sizes
 * the workspace for a batch (grow-only); after it dfot_dit1d_forward allocates nothing and does not synchronise (capturable in a graph).
 * out[B,T,C,1,L] = model(x[B,T,C,1,L], noise_levels[B,T] int32, clamped to [0, timesteps)); tokens must equal max_tokens (DFOT_ERR_SHAPE). */
int dfot_dit1d_create(const dfot_dit1d_config* cfg, dfot_dit1d_t* out);
int dfot_dit1d_destroy(dfot_dit1d_t h);
int dfot_dit1d_num_params(dfot_dit1d_t h);
const char* dfot_dit1d_param_name(dfot_dit1d_t h, int index);
int dfot_dit1d_param_shape(dfot_dit1d_t h, int index, int64_t shape[4], int* ndim);
int dfot_dit1d_load_weight(dfot_dit1d_t h, const char* name, const float* data, const int64_t* shape, int ndim, void* stream);
int dfot_dit1d_finalize(dfot_dit1d_t h, void* stream);
int dfot_dit1d_reserve(dfot_dit1d_t h, int max_batch);
size_t dfot_dit1d_workspace_bytes(dfot_dit1d_t h);
int dfot_dit1d_forward(dfot_dit1d_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens, void* stream);

/* ---- DiT1D training (csrc/dit1d_train.inl; Python mirror: dit1d_trainer.DiT1DTrainer) ----
 * The dfot_dit_train_* contract for the DiT1D backbone: the trainable parameters live in ONE caller-owned flat fp32 buffer with a gradient
 * buffer of the same layout (the reference module's parameters() order, every tensor 16-byte aligned at dfot_dit1d_train_param_offset).
 * pos_embed is a frozen parameter of the reference (requires_grad = False): it is NOT in the flat buffers -- no gradient, no optimizer
 * state, no weight decay -- and is loaded once with dfot_dit1d_train_load_buffer("pos_embed", device fp32 [T * L * hidden]).
 * Limits: those of dfot_dit1d_create, with hidden and mlp_hidden multiples of 128 (the weight-gradient GEMMs tile a feature axis by 128);
 * a violation is DFOT_ERR_SHAPE / DFOT_ERR_ARG with the field's name.  The six modulations of every block are evaluated per frame from
 * the live weights.  attach -> [load_buffer] -> sync_weights (after every parameter update) -> reserve -> forward -> backward (OVERWRITES
 * the gradient buffer with d sum(out * d_out) / d parameter) -> input_grad (d / d x of the same pair).  tokens must equal max_tokens.
 * x must stay alive until backward.  No atomics: two runs give the same bits. */
typedef struct dfot_dit1d_train_s* dfot_dit1d_train_t;
int dfot_dit1d_train_create(const dfot_dit1d_config* cfg, dfot_dit1d_train_t* out);
int dfot_dit1d_train_destroy(dfot_dit1d_train_t h);
int dfot_dit1d_train_num_params(dfot_dit1d_train_t h);
const char* dfot_dit1d_train_param_name(dfot_dit1d_train_t h, int i);
int dfot_dit1d_train_param_shape(dfot_dit1d_train_t h, int i, int64_t shape[4], int* ndim);
int64_t dfot_dit1d_train_param_offset(dfot_dit1d_train_t h, int i);
int64_t dfot_dit1d_train_total_numel(dfot_dit1d_train_t h);
int dfot_dit1d_train_load_buffer(dfot_dit1d_train_t h, const char* name, const float* data, int64_t numel, void* stream);
int dfot_dit1d_train_attach(dfot_dit1d_train_t h, float* params, float* grads);
int dfot_dit1d_train_sync_weights(dfot_dit1d_train_t h, void* stream);
int dfot_dit1d_train_reserve(dfot_dit1d_train_t h, int max_batch);
int dfot_dit1d_train_forward(dfot_dit1d_train_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens, void* stream);
int dfot_dit1d_train_backward(dfot_dit1d_train_t h, const float* d_out, void* stream);
int dfot_dit1d_train_input_grad(dfot_dit1d_train_t h, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFOT_HIP_H_ */
