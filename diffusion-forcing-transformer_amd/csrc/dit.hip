// DiT3D backbone (Kinetics-600 path) on MI355X: weight packing, noise-level modulation table, forward orchestration.
// Mirrors the module tree / state-dict names of the reference
// (algorithms/dfot/backbones/dit/dit3d.py:146-192, dit/dit_base.py:150-196,391-419, dit/dit_blocks.py:49-128,378-542).
//
// Layout: tokens are channels-last rows [B*T*P][hidden]; the residual stream is fp32, GEMM operands bf16.
// Conditioning: c = MLP(sinusoidal(noise level)) depends on the integer level only, and every block consumes it through
// Linear(SiLU(c)).  finalize() therefore evaluates all modulations (shift|scale|gate per AdaLN-Zero, shift|scale for the
// final AdaLN) for every level with ONE GEMM into mod_table[level][...] (1000 x 99072 fp32 = 396 MB at DiT/XL; HBM is
// 288 GB), and forward never touches the embedding MLP or the 228 MB of modulation weights again.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "dfot_hip.h"
#include "dit_model.h"
#include "engine_device.h"
#include "gemm.h"
#include "kernels.h"
#include "level_embed.h"

namespace dfot {
namespace {

typedef __attribute__((ext_vector_type(4))) float float4v;

struct DitBlockW {  // DiTBlock (attn.qkv / attn.proj) or MatrixDiTBlock (the attention factors); norm1, norm2 and the MLP are common
  bf16 *w_qkv = nullptr, *w_proj = nullptr, *w_fc1 = nullptr, *w_fc2 = nullptr;
  float *b_qkv = nullptr, *b_proj = nullptr, *b_fc1 = nullptr, *b_fc2 = nullptr;
  long mod1 = 0, mod2 = 0;  // column offsets of this block's (shift|scale|gate) triples inside a mod_table row
  bf16 *ut = nullptr, *vt = nullptr, *put = nullptr, *pvt = nullptr;  // qkv_u^T [E][P], qkv_v^T [3h][h], proj_u^T [P][E], proj_v^T [h][h]
  float *qkv_bias = nullptr, *proj_bias = nullptr;                      // [E][3h], [P][h]
};

// ---- finalize-time kernels (run once per weight load; the level-embedding ones are level_embed.h) ---------------------
// semb[(flag*lpad + level)][:] = bf16(SiLU(emb[level] + diff_table[flag]))  (DifferenceDiT3D: c = noise emb + diff emb)
__global__ void add_diff_silu_kernel(const float* __restrict__ emb, const float* __restrict__ diff_table, bf16* __restrict__ semb,
                                     int levels, int lpad, int hidden, int flags) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)flags * levels * hidden) return;
  const int c = (int)(i % hidden), lv = (int)((i / hidden) % levels), f = (int)(i / ((long)hidden * levels));
  semb[((long)f * lpad + lv) * hidden + c] = f2bf(silu_f(emb[(long)lv * hidden + c] + diff_table[(long)f * hidden + c]));
}

// dst[c][r] (bf16) = src[r][c] (fp32): weight packing of the matrix factors (stored (in, out) in the reference)
__global__ void pack_transpose_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int rows, int cols) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const int r = (int)(i % rows), c = (int)(i / rows);
  dst[i] = f2bf(src[(long)r * cols + c]);
}

// table row of every (video, token): level + lpad * flag, flag = 1 for difference tokens (even positions of the interleaved
// merge, difference_dit3d.py:159-176 with diff_first=True)
__global__ void make_index_kernel(const int* __restrict__ levels, int* __restrict__ idx, int n, int tokens, int max_level, int lpad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lv = levels[i];
  lv = lv < 0 ? 0 : (lv > max_level ? max_level : lv);
  idx[i] = lv + ((i % tokens) % 2 == 0 ? lpad : 0);
}

// External condition embedding (RandomDropoutCondEmbedding / LabelEmbedding, embeddings.py:364-387) of every (video, token) frame, ONE launch:
//   ce = W2 SiLU(W1 cond + b1) + b2 (action)  |  table[label] (label);   e = base + ce, base = noise-level embedding (+ token-kind
//   embedding of the difference model); frames of a video whose mask byte is set keep e = base;   semb = bf16(SiLU(e)) is the operand
//   of the modulation GEMM, so everything after it is the unconditioned path reading a per-frame table instead of the per-level one.
// One workgroup per frame: the hidden activations of the MLP stay in LDS (hidden floats); fp32 throughout.
struct CondEmbedArgs {
  const float* cond = nullptr;      // action: [frames][cond_dim]
  const int* labels = nullptr;      // label: [frames] table rows (clamped to [0, table_rows))
  const uint8_t* mask = nullptr;    // optional [batch]: 1 = this video runs without its condition
  const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *table = nullptr;
  const float* base = nullptr;      // [..][hidden]: row levels[f] (clamped to max_level) when levels is given, else row f
  const int* levels = nullptr;
  const float* diff_table = nullptr;  // optional [2][hidden]: row 1 for even (difference) tokens, row 0 for odd ones
  float* e_out = nullptr;           // optional fp32 [frames][hidden] (may alias base when levels == nullptr: each element is read, then written)
  bf16* semb = nullptr;             // [frames][hidden]
  float *h1_out = nullptr, *a1_out = nullptr;  // optional (training): pre-activation and SiLU output of the first Linear
  int* idx = nullptr;               // optional [frames]: idx[f] = f, the row of frame f in the per-frame modulation table
  int tokens = 0, cond_dim = 0, hidden = 0, table_rows = 0, max_level = 0;
};

template <bool LABEL>
__global__ __launch_bounds__(256) void cond_embed_kernel(const CondEmbedArgs a) {
  extern __shared__ float act[];  // [hidden]: SiLU(W1 cond + b1)
  const int f = blockIdx.x, b = f / a.tokens, t = f % a.tokens, hidden = a.hidden;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool masked = a.mask && a.mask[b];
  long brow = f;
  if (a.levels) {
    int lv = a.levels[f];
    brow = lv < 0 ? 0 : (lv > a.max_level ? a.max_level : lv);
  }
  const float* base = a.base + brow * hidden;
  const float* diff = a.diff_table ? a.diff_table + (long)(t % 2 == 0 ? 1 : 0) * hidden : nullptr;
  auto finish = [&](int o, float ce) {
    float e = base[o];
    if (diff) e += diff[o];
    if (!masked) e += ce;
    if (a.e_out) a.e_out[(long)f * hidden + o] = e;
    a.semb[(long)f * hidden + o] = f2bf(silu_f(e));
  };
  if (threadIdx.x == 0 && a.idx) a.idx[f] = f;
  if constexpr (LABEL) {
    int row = a.labels[f];
    row = row < 0 ? 0 : (row >= a.table_rows ? a.table_rows - 1 : row);
    for (int o = threadIdx.x; o < hidden; o += 256) finish(o, a.table[(long)row * hidden + o]);
  } else {
    const float* cv = a.cond + (long)f * a.cond_dim;
    for (int o = threadIdx.x; o < hidden; o += 256) {
      float acc = 0.f;
      for (int k = 0; k < a.cond_dim; ++k) acc += a.w1[(long)o * a.cond_dim + k] * cv[k];
      acc += a.b1[o];
      const float s = silu_f(acc);
      act[o] = s;
      if (a.h1_out) a.h1_out[(long)f * hidden + o] = acc;
      if (a.a1_out) a.a1_out[(long)f * hidden + o] = s;
    }
    __syncthreads();
    for (int o = wave; o < hidden; o += 4) {  // one wave per output channel, as rows_linear_kernel
      float acc = 0.f;
      for (int i = lane; i < hidden; i += 64) acc += a.w2[(long)o * hidden + i] * act[i];
      acc = wave_sum(acc);
      if (lane == 0) finish(o, acc + a.b2[o]);
    }
  }
}

int launch_cond_embed(const CondEmbedArgs& a, int frames, hipStream_t s) {
  if (a.labels)
    hipLaunchKernelGGL(cond_embed_kernel<true>, dim3(frames), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(cond_embed_kernel<false>, dim3(frames), dim3(256), a.hidden * sizeof(float), s, a);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// ---- continuous diffusion front end (cfg.fourier_noise) -----------------------------------------------------------------
// FourierEmbedding (embeddings.py:94-109): sqrt(2) * cos(level * freq + phase), fp32.  The reference forms the argument with one rounded
// multiply and one rounded add (two torch ops), so no FMA here: at |level * freq| of tens of radians one ulp of the argument is 4e-6.
// cosf is the accurately range-reduced one (not __cosf); the scale is float(sqrt(2)), as torch multiplies an fp32 tensor by a Python scalar.
// (__fmul_rn / __fadd_rn are plain operators in HIP's headers and would be contracted: the pragma is what keeps the two roundings.)
__device__ __forceinline__ float fourier_feature(float level, float freq, float phase) {
#pragma clang fp contract(off)
  const float m = level * freq;
  const float a = m + phase;
  return cosf(a) * 1.41421356237309515f;
}

__global__ void fourier_features_kernel(const float* __restrict__ levels, const float* __restrict__ freqs, const float* __restrict__ phases,
                                        float* __restrict__ feat, int frames, int dim) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)frames * dim) return;
  const int c = (int)(i % dim);
  feat[i] = fourier_feature(levels[i / dim], freqs[c], phases[c]);
}

// The noise-level embedding of the frames, fp32 on the VALU: features -> Linear -> SiLU (fourier_hidden_kernel) -> Linear (fourier_out_kernel).
// The two linears run over B*T rows (5..128): a 256-row MFMA tile would be >= 50 % padding and would round the operands to bf16, while the
// table path this replaces evaluates them in fp32 (rows_linear_kernel), so this keeps its arithmetic -- one wave per output channel, lanes
// strided over K, xor-shuffle sum, i.e. the summation order of rows_linear_kernel.  A workgroup owns FE_FRAMES frames x FE_COLS output
// channels, so each weight row is read once per FE_FRAMES frames and the grid (frame groups x channel chunks) covers the chip.  Every
// frame's sums are formed in an order that does not depend on its neighbours: a video gives the same bits alone and in a batch.
//   act [frames][hidden] = SiLU(linear_1(feat)) (workspace);  n_out [frames][hidden] = linear_2(act);  feat_out [frames][dim] (tap "noise_feat")
//   semb != nullptr (no external condition follows): e = n (+ diff_table[token kind]) -> n_out, semb = bf16(SiLU(e)), idx[f] = f
constexpr int FE_FRAMES = 4, FE_COLS = 32;
struct FourierEmbedArgs {
  const float *levels = nullptr, *freqs = nullptr, *phases = nullptr;
  const float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
  const float* diff_table = nullptr;  // optional [2][hidden]: row 1 for even (difference) tokens
  float *feat_out = nullptr, *act = nullptr, *n_out = nullptr;
  bf16* semb = nullptr;
  int* idx = nullptr;
  int frames = 0, tokens = 0, dim = 0, hidden = 0;
};

// out[r] for the FE_FRAMES rows `in` (LDS, row stride kdim) of output channel o: lane r < FE_FRAMES returns row r's sum
__device__ __forceinline__ float fe_rows_dot(const float* __restrict__ w, const float* in, int kdim, int lane) {
  float acc[FE_FRAMES];
#pragma unroll
  for (int r = 0; r < FE_FRAMES; ++r) acc[r] = 0.f;
  for (int i = lane; i < kdim; i += 64) {
    const float wv = w[i];
#pragma unroll
    for (int r = 0; r < FE_FRAMES; ++r) acc[r] += wv * in[r * kdim + i];
  }
  float v = 0.f;
#pragma unroll
  for (int r = 0; r < FE_FRAMES; ++r) {
    const float t = wave_sum(acc[r]);
    v = lane == r ? t : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void fourier_hidden_kernel(const FourierEmbedArgs a) {
  extern __shared__ float fe_lds[];  // feat [FE_FRAMES][dim]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = blockIdx.x * FE_FRAMES, o0 = blockIdx.y * FE_COLS, dim = a.dim, hidden = a.hidden;
  for (int i = threadIdx.x; i < FE_FRAMES * dim; i += 256) {
    const int r = i / dim, c = i % dim, f = f0 + r;
    float v = 0.f;
    if (f < a.frames) {
      v = fourier_feature(a.levels[f], a.freqs[c], a.phases[c]);
      if (blockIdx.y == 0) a.feat_out[(long)f * dim + c] = v;
    }
    fe_lds[i] = v;
  }
  __syncthreads();
  for (int o = o0 + wave; o < o0 + FE_COLS && o < hidden; o += 4) {
    const float v = fe_rows_dot(a.w1 + (long)o * dim, fe_lds, dim, lane);
    if (lane < FE_FRAMES && f0 + lane < a.frames) a.act[(long)(f0 + lane) * hidden + o] = silu_f(v + a.b1[o]);
  }
}

__global__ __launch_bounds__(256) void fourier_out_kernel(const FourierEmbedArgs a) {
  extern __shared__ float fe_lds[];  // act [FE_FRAMES][hidden]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = blockIdx.x * FE_FRAMES, o0 = blockIdx.y * FE_COLS, hidden = a.hidden;
  for (int i = threadIdx.x; i < FE_FRAMES * hidden; i += 256) {
    const int f = f0 + i / hidden;
    fe_lds[i] = f < a.frames ? a.act[(long)f * hidden + i % hidden] : 0.f;
  }
  __syncthreads();
  for (int o = o0 + wave; o < o0 + FE_COLS && o < hidden; o += 4) {
    const float v = fe_rows_dot(a.w2 + (long)o * hidden, fe_lds, hidden, lane);
    const int f = f0 + lane;
    if (lane < FE_FRAMES && f < a.frames) {
      float e = v + a.b2[o];
      if (a.semb) {
        if (a.diff_table) e += a.diff_table[(long)((f % a.tokens) % 2 == 0 ? 1 : 0) * hidden + o];
        a.semb[(long)f * hidden + o] = f2bf(silu_f(e));
      }
      a.n_out[(long)f * hidden + o] = e;
    }
  }
  if (a.idx && blockIdx.y == 0 && threadIdx.x < FE_FRAMES && f0 + threadIdx.x < a.frames) a.idx[f0 + threadIdx.x] = f0 + threadIdx.x;
}

int launch_fourier_embed(const FourierEmbedArgs& a, hipStream_t s) {
  const dim3 grid(cdiv(a.frames, FE_FRAMES), cdiv(a.hidden, FE_COLS));  // LDS <= 32 KB: noise_dim <= 2048 and hidden <= 2048 at create
  hipLaunchKernelGGL(fourier_hidden_kernel, grid, dim3(256), (size_t)FE_FRAMES * a.dim * sizeof(float), s, a);
  hipLaunchKernelGGL(fourier_out_kernel, grid, dim3(256), (size_t)FE_FRAMES * a.hidden * sizeof(float), s, a);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// per-frame 2-D transpose of a bf16 matrix: src [frames][R][C] -> dst [frames][C][R]; 64x64 tiles through LDS
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, int R, int C) {
  __shared__ bf16 tile[64][66];
  const long f = blockIdx.z;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const bf16* s = src + f * R * C;
  bf16* d = dst + f * R * C;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[ty * 16 + i][tx] = s[(long)(r0 + ty * 16 + i) * C + c0 + tx];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) d[(long)(c0 + ty * 16 + i) * R + r0 + tx] = tile[tx][ty * 16 + i];
}

// MatrixAttention core (dit_blocks.py:289-336, multi_token = False, no RoPE): every frame is one token whose q/k/v are
// (hn x hd) matrices; z [B*L*E][3h] holds (q|k|v) with columns (row head r, d) and rows (frame, col head c, n).
// One workgroup per (video, c, r): scores L x L = scale * <q_l, k_l'> over the hn*hd entries, softmax over l', o = P v.
// o [B*L*E][h] in the same row/column order.
// LT > 0: L == LT is a compile-time constant and every thread keeps the L x L partial scores of its slice of the hn*hd
// entries in registers (each q/k/v entry is read exactly once); LT == 0: generic L <= 32 (one pair of tokens per wave pass).
template <int LT>
__global__ __launch_bounds__(256) void matrix_attn_kernel(const bf16* __restrict__ z, bf16* __restrict__ o, int L, int E, int h,
                                                          int cc, int rr, float scale) {
  __shared__ float sc[32 * 32];
  __shared__ float part[4][LT > 0 ? LT * LT : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / (cc * rr), c = (blockIdx.x / rr) % cc, r = blockIdx.x % rr;
  const int hn = E / cc, hd = h / rr, ne = hn * hd / 4;
  const long ldz = 3L * h;
  auto zrow = [&](int l, int n) { return z + (((long)b * L + l) * E + c * hn + n) * ldz + r * hd; };
  if constexpr (LT > 0) {
    float acc[LT * LT];
#pragma unroll
    for (int i = 0; i < LT * LT; ++i) acc[i] = 0.f;
    for (int e = threadIdx.x; e < ne; e += 256) {
      const int n = (e * 4) / hd, d = (e * 4) % hd;
      float q[LT][4], k[LT][4];
#pragma unroll
      for (int l = 0; l < LT; ++l) {
        const bf16* p = zrow(l, n) + d;
        const bf16x4 q4 = *reinterpret_cast<const bf16x4*>(p);
        const bf16x4 k4 = *reinterpret_cast<const bf16x4*>(p + h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          q[l][j] = bf2f(q4[j]);
          k[l][j] = bf2f(k4[j]);
        }
      }
#pragma unroll
      for (int l = 0; l < LT; ++l)
#pragma unroll
        for (int l2 = 0; l2 < LT; ++l2)
          acc[l * LT + l2] += (q[l][0] * k[l2][0] + q[l][1] * k[l2][1]) + (q[l][2] * k[l2][2] + q[l][3] * k[l2][3]);
    }
#pragma unroll
    for (int i = 0; i < LT * LT; ++i) {
      const float t = wave_sum(acc[i]);
      if (lane == 0) part[wave][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < LT * LT) sc[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]) * scale;
  } else {
    for (int pi = wave; pi < L * L; pi += 4) {
      const int l = pi / L, l2 = pi % L;
      float acc = 0.f;
      for (int e = lane; e < ne; e += 64) {
        const int n = (e * 4) / hd, d = (e * 4) % hd;
        const bf16x4 q4 = *reinterpret_cast<const bf16x4*>(zrow(l, n) + d);
        const bf16x4 k4 = *reinterpret_cast<const bf16x4*>(zrow(l2, n) + h + d);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += bf2f(q4[j]) * bf2f(k4[j]);
      }
      acc = wave_sum(acc);
      if (lane == 0) sc[pi] = acc * scale;
    }
  }
  __syncthreads();
  if (threadIdx.x < L) {
    float* row = sc + threadIdx.x * L;
    float mx = row[0];
    for (int j = 1; j < L; ++j) mx = fmaxf(mx, row[j]);
    float sum = 0.f;
    for (int j = 0; j < L; ++j) {
      row[j] = __expf(row[j] - mx);
      sum += row[j];
    }
    const float inv = 1.0f / sum;
    for (int j = 0; j < L; ++j) row[j] *= inv;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ne; e += 256) {
    const int n = (e * 4) / hd, d = (e * 4) % hd;
    if constexpr (LT > 0) {
      float v[LT][4];
#pragma unroll
      for (int l2 = 0; l2 < LT; ++l2) {
        const bf16x4 v4 = *reinterpret_cast<const bf16x4*>(zrow(l2, n) + 2 * h + d);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[l2][j] = bf2f(v4[j]);
      }
#pragma unroll
      for (int l = 0; l < LT; ++l) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int l2 = 0; l2 < LT; ++l2) {
          const float pw = sc[l * LT + l2];
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += pw * v[l2][j];
        }
        bf16x4 o4;
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = f2bf(a[j]);
        *reinterpret_cast<bf16x4*>(o + (((long)b * LT + l) * E + c * hn + n) * h + r * hd + d) = o4;
      }
    } else {
      for (int l = 0; l < L; ++l) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int l2 = 0; l2 < L; ++l2) {
          const bf16x4 v4 = *reinterpret_cast<const bf16x4*>(zrow(l2, n) + 2 * h + d);
          const float pw = sc[l * L + l2];
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += pw * bf2f(v4[j]);
        }
        bf16x4 o4;
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = f2bf(a[j]);
        *reinterpret_cast<bf16x4*>(o + (((long)b * L + l) * E + c * hn + n) * h + r * hd + d) = o4;
      }
    }
  }
}

int launch_matrix_attn(const bf16* z, bf16* o, int batch, int L, int E, int h, int cc, int rr, float scale, hipStream_t s) {
  DFOT_REQUIRE(L > 0 && L <= 32, DFOT_ERR_SHAPE, "matrix attention: %d frame tokens (max 32)", L);
  const dim3 grid(batch * cc * rr), blk(256);
  switch (L) {
    case 2: hipLaunchKernelGGL(matrix_attn_kernel<2>, grid, blk, 0, s, z, o, L, E, h, cc, rr, scale); break;
    case 4: hipLaunchKernelGGL(matrix_attn_kernel<4>, grid, blk, 0, s, z, o, L, E, h, cc, rr, scale); break;
    case 6: hipLaunchKernelGGL(matrix_attn_kernel<6>, grid, blk, 0, s, z, o, L, E, h, cc, rr, scale); break;
    case 8: hipLaunchKernelGGL(matrix_attn_kernel<8>, grid, blk, 0, s, z, o, L, E, h, cc, rr, scale); break;
    case 10: hipLaunchKernelGGL(matrix_attn_kernel<10>, grid, blk, 0, s, z, o, L, E, h, cc, rr, scale); break;
    default: hipLaunchKernelGGL(matrix_attn_kernel<0>, grid, blk, 0, s, z, o, L, E, h, cc, rr, scale); break;
  }
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// ---- forward kernels --------------------------------------------------------------------------------------------
// x[(b, t, p)][:] += tpos[t][:]: the temporal half of sinusoidal_factorized, added once after spatial block 0 (dit_base.py:408-411)
__global__ __launch_bounds__(256) void add_temporal_pos_kernel(float* __restrict__ x, const float* __restrict__ tpos, int tokens, int P,
                                                               int hidden4, long total4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)(i % hidden4), t = (int)((i / ((long)hidden4 * P)) % tokens);
  float4v* xp = reinterpret_cast<float4v*>(x) + i;
  *xp = *xp + reinterpret_cast<const float4v*>(tpos)[(long)t * hidden4 + c];
}

// PatchEmbed (Conv2d k = s = p): x [BT][C][H][W] fp32 -> tokens [BT*gh*gw][hidden] fp32.  8 tokens per workgroup so each
// weight row is fetched once per 8 tokens; thread = output channels t, t+256, ...
constexpr int PE_TOK = 8;
__global__ __launch_bounds__(256) void patch_embed_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ b, const float* __restrict__ pos,
                                                          float* __restrict__ out, int c, int hh, int ww, int ps, int hidden,
                                                          long rows) {
  extern __shared__ float patch[];  // [PE_TOK][kdim]
  const int gh = hh / ps, gw = ww / ps, kdim = c * ps * ps;
  const long row0 = (long)blockIdx.x * PE_TOK;
  for (int i = threadIdx.x; i < PE_TOK * kdim; i += 256) {
    const long row = row0 + i / kdim;
    const int kk = i % kdim;  // (ci, py, px) -- the Conv2d weight's own flattening
    float v = 0.f;
    if (row < rows) {
      const long bt = row / (gh * gw);
      const int g = (int)(row % (gh * gw)), gy = g / gw, gx = g % gw;
      const int ci = kk / (ps * ps), py = (kk / ps) % ps, px = kk % ps;
      v = x[((bt * c + ci) * hh + gy * ps + py) * ww + gx * ps + px];
    }
    patch[i] = v;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < hidden; o += 256) {
    float acc[PE_TOK];
    const float bias = b[o];
#pragma unroll
    for (int t = 0; t < PE_TOK; ++t) acc[t] = bias;
    for (int kk = 0; kk < kdim; ++kk) {
      const float wv = w[(long)o * kdim + kk];
#pragma unroll
      for (int t = 0; t < PE_TOK; ++t) acc[t] += wv * patch[t * kdim + kk];
    }
#pragma unroll
    for (int t = 0; t < PE_TOK; ++t)
      if (row0 + t < rows)  // pos: optional absolute positional embedding [P][hidden] of the token's patch (sinusoidal_2d)
        out[(row0 + t) * hidden + o] = acc[t] + (pos ? pos[((row0 + t) % (gh * gw)) * hidden + o] : 0.f);
  }
}

// AdaLN: m = LayerNorm(x) * (1 + scale) + shift, (shift|scale) = mod_table[level of the row's frame][off ...].
// One wave per token row; a lane owns CNT groups of VEC consecutive channels (hidden = 64 * VEC * CNT, compile-time so the
// row lives in registers without guards).  Writes m as fp32 (the block's residual base, in place) and bf16 (GEMM operand).
template <int VEC>
struct VecT;
template <>
struct VecT<1> { typedef float type; };
template <>
struct VecT<2> { typedef __attribute__((ext_vector_type(2))) float type; };
template <>
struct VecT<4> { typedef __attribute__((ext_vector_type(4))) float type; };
template <int VEC>
struct BVecT;
template <>
struct BVecT<1> { typedef bf16 type; };
template <>
struct BVecT<2> { typedef bf16x2 type; };
template <>
struct BVecT<4> { typedef bf16x4 type; };

template <int VEC>
__device__ __forceinline__ float vsum(const typename VecT<VEC>::type& v) {
  if constexpr (VEC == 1) return v;
  else if constexpr (VEC == 2) return v[0] + v[1];
  else return (v[0] + v[1]) + (v[2] + v[3]);
}
template <int VEC>
__device__ __forceinline__ float vdot(const typename VecT<VEC>::type& a, const typename VecT<VEC>::type& b) {
  if constexpr (VEC == 1) return a * b;
  else if constexpr (VEC == 2) return a[0] * b[0] + a[1] * b[1];
  else return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

// normalised + modulated row in registers: v[i] covers channels (i*64 + lane)*VEC ...
template <int VEC, int CNT>
__device__ __forceinline__ void ln_mod_row(const float* __restrict__ xr, const float* __restrict__ sh, int hidden, float eps,
                                           int lane, typename VecT<VEC>::type (&v)[CNT]) {
  typedef typename VecT<VEC>::type V;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CNT; ++i) {
    v[i] = *reinterpret_cast<const V*>(xr + (i * 64 + lane) * VEC);
    s += vsum<VEC>(v[i]);
  }
  const float mean = wave_sum(s) / (float)hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < CNT; ++i) {
    v[i] -= mean;
    q += vdot<VEC>(v[i], v[i]);
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)hidden + eps);
  const float* sc = sh + hidden;
#pragma unroll
  for (int i = 0; i < CNT; ++i) {
    const V a = *reinterpret_cast<const V*>(sh + (i * 64 + lane) * VEC);
    const V g = *reinterpret_cast<const V*>(sc + (i * 64 + lane) * VEC);
    v[i] = v[i] * rstd * (1.0f + g) + a;
  }
}

template <int VEC, int CNT>
__global__ __launch_bounds__(256) void ln_mod_kernel(const float* xin, float* xout, bf16* __restrict__ obf,
                                                     const float* __restrict__ table, const int* __restrict__ levels,
                                                     long ldt, long off, int rows_per_frame, int rows, float eps,
                                                     int max_level) {
  typedef typename VecT<VEC>::type V;
  typedef typename BVecT<VEC>::type B;
  constexpr int hidden = 64 * VEC * CNT;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* xr = xout + (long)row * hidden;  // xout may alias xin (inference: in place); training keeps x for the backward
  int lv = levels[row / rows_per_frame];
  lv = lv < 0 ? 0 : (lv > max_level ? max_level : lv);
  V v[CNT];
  ln_mod_row<VEC, CNT>(xin + (long)row * hidden, table + (long)lv * ldt + off, hidden, eps, lane, v);
  bf16* orow = obf + (long)row * hidden;
#pragma unroll
  for (int i = 0; i < CNT; ++i) {
    *reinterpret_cast<V*>(xr + (i * 64 + lane) * VEC) = v[i];
    B o;
    if constexpr (VEC == 1) {
      o = f2bf(v[i]);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = f2bf(v[i][j]);
    }
    *reinterpret_cast<B*>(orow + (i * 64 + lane) * VEC) = o;
  }
}

// Final layer: AdaLN (shift|scale) -> Linear(hidden, p*p*C) -> unpatchify to [BT][C][H][W] (dit3d.py:129-144).
// One wave per token row; the weight (oc x hidden fp32, 72 KB at K600) is staged in LDS once per workgroup of FIN_ROWS rows.
constexpr int FIN_ROWS = 16;
constexpr int FIN_LDS_BYTES = 160 * 1024;  // the whole LDS of a CU
template <int VEC, int CNT>
__global__ __launch_bounds__(256) void final_layer_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                          const int* __restrict__ levels, long ldt, long off,
                                                          const float* __restrict__ w, const float* __restrict__ b,
                                                          float* __restrict__ out, int rows_per_frame, int rows, float eps,
                                                          int max_level, int c, int hh, int ww, int ps) {
  typedef typename VecT<VEC>::type V;
  constexpr int hidden = 64 * VEC * CNT;
  extern __shared__ float wl[];  // [oc][hidden]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int oc = ps * ps * c;
  for (int i = threadIdx.x * 4; i < oc * hidden; i += 1024)
    *reinterpret_cast<float4v*>(wl + i) = *reinterpret_cast<const float4v*>(w + i);
  __syncthreads();
  const int gw = ww / ps;
  for (int rr = wave; rr < FIN_ROWS; rr += 4) {
    const int row = blockIdx.x * FIN_ROWS + rr;
    if (row >= rows) break;
    const int bt = row / rows_per_frame;
    int lv = levels[bt];
    lv = lv < 0 ? 0 : (lv > max_level ? max_level : lv);
    V v[CNT];
    ln_mod_row<VEC, CNT>(x + (long)row * hidden, table + (long)lv * ldt + off, hidden, eps, lane, v);
    const int g = row % rows_per_frame, gy = g / gw, gx = g % gw;
    for (int o = 0; o < oc; ++o) {  // o = (p, q, channel), channel fastest
      const float* wr = wl + o * hidden;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < CNT; ++i) acc += vdot<VEC>(v[i], *reinterpret_cast<const V*>(wr + (i * 64 + lane) * VEC));
      acc = wave_sum(acc);
      if (lane == 0) {
        const int ch = o % c, pq = o / c, py = pq / ps, px = pq % ps;
        out[(((long)bt * c + ch) * hh + gy * ps + py) * ww + gx * ps + px] = acc + b[o];
      }
    }
  }
}

// The same layer for a weight that does not fit in LDS (DiT/B at the 32-channel Minecraft / dmlab latents: 128 x 768 fp32 = 384 KB): the
// weight streams through LDS in chunks of `chunk` output rows, each chunk used by all FIN_ROWS rows of the workgroup.  The row loop is
// final_layer_kernel's own, statement for statement, so that the compiler forms the same multiplies and adds (which products it fuses
// follows the loop's shape: with a wave's four rows held in registers across the chunks it fused differently and outputs moved by an
// ulp); a row is therefore normalised again for every chunk, one more read of a row that is in L2.  Same bits as final_layer_kernel.
template <int VEC, int CNT>
__global__ __launch_bounds__(256) void final_layer_chunked_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                                  const int* __restrict__ levels, long ldt, long off,
                                                                  const float* __restrict__ w, const float* __restrict__ b,
                                                                  float* __restrict__ out, int rows_per_frame, int rows, float eps,
                                                                  int max_level, int c, int hh, int ww, int ps, int chunk) {
  typedef typename VecT<VEC>::type V;
  constexpr int hidden = 64 * VEC * CNT;
  extern __shared__ float wl[];  // [chunk][hidden]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int oc = ps * ps * c;
  const int gw = ww / ps;
  for (int o0 = 0; o0 < oc; o0 += chunk) {
    const int n = oc - o0 < chunk ? oc - o0 : chunk;
    if (o0) __syncthreads();  // every wave is done with the previous chunk
    const float* wc = w + (long)o0 * hidden;
    for (int i = threadIdx.x * 4; i < n * hidden; i += 1024)
      *reinterpret_cast<float4v*>(wl + i) = *reinterpret_cast<const float4v*>(wc + i);
    __syncthreads();
    for (int rr = wave; rr < FIN_ROWS; rr += 4) {
      const int row = blockIdx.x * FIN_ROWS + rr;
      if (row >= rows) break;
      const int bt = row / rows_per_frame;
      int lv = levels[bt];
      lv = lv < 0 ? 0 : (lv > max_level ? max_level : lv);
      V v[CNT];
      ln_mod_row<VEC, CNT>(x + (long)row * hidden, table + (long)lv * ldt + off, hidden, eps, lane, v);
      const int g = row % rows_per_frame, gy = g / gw, gx = g % gw;
      for (int oo = 0; oo < n; ++oo) {
        const int o = o0 + oo;  // o = (p, q, channel), channel fastest
        const float* wr = wl + oo * hidden;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < CNT; ++i) acc += vdot<VEC>(v[i], *reinterpret_cast<const V*>(wr + (i * 64 + lane) * VEC));
        acc = wave_sum(acc);
        if (lane == 0) {
          const int ch = o % c, pq = o / c, py = pq / ps, px = pq % ps;
          out[(((long)bt * c + ch) * hh + gy * ps + py) * ww + gx * ps + px] = acc + b[o];
        }
      }
    }
  }
}

// hidden = 64 * VEC * CNT with VEC = 2 when hidden % 128 == 0 (8-byte accesses), else 1
#define DIT_LN_DISPATCH(CALL)                                 \
  switch (hidden % 128 == 0 ? hidden / 128 : hidden % 64 == 0 ? -(hidden / 64) : 0) { \
    case 1: CALL(2, 1); break;                                 \
    case 2: CALL(2, 2); break;                                 \
    case 3: CALL(2, 3); break;                                 \
    case 4: CALL(2, 4); break;                                 \
    case 5: CALL(2, 5); break;                                 \
    case 6: CALL(2, 6); break;                                 \
    case 7: CALL(2, 7); break;                                 \
    case 8: CALL(2, 8); break;                                 \
    case 9: CALL(2, 9); break;                                 \
    case 10: CALL(2, 10); break;                               \
    case 12: CALL(2, 12); break;                               \
    case 16: CALL(2, 16); break;                               \
    case -1: CALL(1, 1); break;                                \
    case -3: CALL(1, 3); break;                                \
    case -5: CALL(1, 5); break;                                \
    case -7: CALL(1, 7); break;                                \
    case -9: CALL(1, 9); break;                                \
    default:                                                   \
      set_error("DiT: hidden size %d has no LayerNorm kernel instance", hidden); \
      return DFOT_ERR_SHAPE;                                   \
  }

int launch_ln_mod(const float* xin, float* x, bf16* obf, const float* table, const int* levels, long ldt, long off, int hidden, int rows_per_frame,
                  int rows, float eps, int max_level, hipStream_t s) {
#define CALL(V, C) \
  hipLaunchKernelGGL((ln_mod_kernel<V, C>), dim3(cdiv(rows, 4)), dim3(256), 0, s, xin, x, obf, table, levels, ldt, off, rows_per_frame, rows, eps, max_level)
  DIT_LN_DISPATCH(CALL)
#undef CALL
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// the patch embedding of both engines (inference forward, training forward): 8 token rows per workgroup
int launch_patch_embed(const float* x, const float* w, const float* b, const float* pos, float* out, int c, int hh, int ww, int ps, int hidden,
                       long rows, hipStream_t s) {
  hipLaunchKernelGGL(patch_embed_kernel, dim3(cdiv(rows, PE_TOK)), dim3(256), PE_TOK * c * ps * ps * sizeof(float), s, x, w, b, pos, out, c, hh, ww,
                     ps, hidden, rows);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int launch_final_layer(const float* x, const float* table, const int* levels, long ldt, long off, const float* w, const float* b,
                       float* out, int hidden, int rows_per_frame, int rows, float eps, int max_level, int c, int hh, int ww, int ps,
                       hipStream_t s, int form = 0, int chunk = 0) {
  // form 0: the LDS-resident kernel whenever the weight fits (every model that ran before the chunked form existed launches what it
  // launched then), else the chunked one; 1: LDS-resident or an error; 2: chunked, `chunk` output rows at a time (0 = what fits)
  const int oc = ps * ps * c;
  const int lds = oc * hidden * (int)sizeof(float);
  if (form == 2 || (form == 0 && lds > FIN_LDS_BYTES)) {
    DFOT_REQUIRE(hidden > 0 && (long)hidden * sizeof(float) <= FIN_LDS_BYTES, DFOT_ERR_SHAPE, "final layer: hidden size %d", hidden);
    const int fit = FIN_LDS_BYTES / (hidden * (int)sizeof(float));
    DFOT_REQUIRE(chunk >= 0 && chunk <= fit, DFOT_ERR_ARG, "final layer: chunk of %d output rows (at most %d fit in LDS)", chunk, fit);
    int ch = chunk ? chunk : fit;
    ch = ch < oc ? ch : oc;
    const int clds = ch * hidden * (int)sizeof(float);
#define CALL(V, C)                                                                                                          \
  {                                                                                                                         \
    auto kern = final_layer_chunked_kernel<V, C>;                                                                           \
    static int lds_set = 0; /* once per instantiation and size (not inside a captured step) */                                \
    if (lds_set < clds) {                                                                                                   \
      DFOT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, clds)); \
      lds_set = clds;                                                                                                       \
    }                                                                                                                       \
    hipLaunchKernelGGL(kern, dim3(cdiv(rows, FIN_ROWS)), dim3(256), clds, s, x, table, levels, ldt, off, w, b, out, rows_per_frame, \
                       rows, eps, max_level, c, hh, ww, ps, ch);                                                            \
  }
    DIT_LN_DISPATCH(CALL)
#undef CALL
    DFOT_CHECK_HIP(hipGetLastError());
    return DFOT_OK;
  }
  DFOT_REQUIRE(form == 0 || form == 1, DFOT_ERR_ARG, "final layer: form %d (0 = automatic, 1 = LDS-resident, 2 = chunked)", form);
  DFOT_REQUIRE(lds <= FIN_LDS_BYTES, DFOT_ERR_SHAPE, "final layer: weight (%d B) does not fit in LDS", lds);
#define CALL(V, C)                                                                                                        \
  {                                                                                                                         \
    auto kern = final_layer_kernel<V, C>;                                                                                   \
    static int lds_set = 0; /* once per instantiation and size (not inside a captured step) */                                \
    if (lds_set < lds) {                                                                                                    \
      DFOT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds)); \
      lds_set = lds;                                                                                                        \
    }                                                                                                                       \
    hipLaunchKernelGGL(kern, dim3(cdiv(rows, FIN_ROWS)), dim3(256), lds, s, x, table, levels, ldt, off, w, b, out, rows_per_frame, \
                       rows, eps, max_level, c, hh, ww, ps);                                                                \
  }
  DIT_LN_DISPATCH(CALL)
#undef CALL
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace
}  // namespace dfot

using namespace dfot;

struct dfot_dit_s : DitGeom, EngineDevice {  // the geometry of cfg (dit_model.h): gh, gw, P, d, dstride, kpatch, oc, c_rows, ldt, mod_final
  dfot_dit_s() : EngineDevice("") {}
  DitCfg cfg{};
  int lpad = 0;      // level count padded to the GEMM's row tile
  // weights
  float *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr, *pe_w = nullptr, *pe_b = nullptr,
        *fin_w = nullptr, *fin_b = nullptr, *b_mod = nullptr;
  bf16* w_mod = nullptr;  // every modulation Linear stacked: [ldt][hidden]
  std::vector<DitBlockW> blocks;
  std::vector<DitBlockW> tblocks;   // variants 1 and 3: one MatrixDiTBlock after every spatial block
  std::vector<DitBlockW> fblocks;   // variant 2: one temporal DiTBlock after every spatial block
  float *diff_table = nullptr, *pos2d = nullptr, *tpos = nullptr;  // tpos: variant 2, temporal sinusoidal table [max_tokens][hidden]
  float* trope = nullptr;  // variant 3 with use_temporal_rope: (cos, sin) [max_tokens][hd/2][2] of the matrix attention's RoPE-1D
  float *c_w1 = nullptr, *c_b1 = nullptr, *c_w2 = nullptr, *c_b2 = nullptr, *c_table = nullptr;  // external condition embedding
  float *fz_freqs = nullptr, *fz_phases = nullptr;  // fourier_noise: the FourierEmbedding buffers [noise_dim]
  int mod_variant = GEMM_AUTO;       // GEMM tile form finalize() used for mod_table: the per-frame table uses the same one (bit-identical rows)
  // derived at finalize
  float *freqs = nullptr, *feat = nullptr, *thid = nullptr, *emb = nullptr, *mod_table = nullptr, *rope_cs = nullptr;
  bf16* semb = nullptr;
  bool finalized = false;
  // workspace
  int max_batch = 0, last_rows = 0;
  float* X = nullptr;
  bf16 *A = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *hid = nullptr;
  bf16 *T1 = nullptr, *W1 = nullptr, *W2 = nullptr, *Z = nullptr;  // variant 1: transposes / left-factor products / qkv of frames
  int* idx = nullptr;                                              // variant 1: mod_table row per (video, token)
  // conditioned forward: per-frame SiLU(embedding), modulation table [fpad][ldt] and its row index; e of the last call (tap "cond_emb")
  int fpad = 0, last_cond_frames = 0;
  bf16* csemb = nullptr;
  float *cmod = nullptr, *cemb = nullptr;
  int* cidx = nullptr;
  float* nfeat = nullptr;  // fourier_noise: Fourier features of the last forward [frames][noise_dim] (tap "noise_feat")
  float* nact = nullptr;   // fourier_noise: SiLU(linear_1(features)) [frames][hidden]
  int last_feat_frames = 0;
  int gemm_variant = GEMM_AUTO;
  bool time_attn = false;
  bool front_only = false;  // measurement: forward returns once the modulations of the call are formed (tools/bench_ops.py dit_front)
  std::vector<hipEvent_t> ev_start, ev_stop;
  size_t ev_used = 0;
  // attention-map capture (dfot_dit_capture_attention); off unless cap_form >= 0.  The buffers are owned apart from the workspace
  int cap_form = DFOT_ATTN_MAP_OFF;
  std::vector<int> cap_blocks;        // selected frame-mixing blocks, ascending
  size_t cap_max_bytes = 0, cap_bytes = 0;
  std::vector<float*> cap_maps;       // one per selected block, sized for max_batch x max_tokens
  float* cap_part = nullptr;          // partial sums of the frame form (shared by the blocks: same stream)
  int cap_batch = 0, cap_tokens = 0;  // batch / tokens of the last forward that captured (0: none yet)
};

namespace dfot {
namespace {

// the loader of an inventory entry (dit_model.h) that only this engine has (the others: engine_device.h): dst[c][r] bf16 = src[r][c].
// The matrix factors are stored (in, out); the GEMMs want [out][in]
int dit_add_transposed(dfot_dit_s* h, const DitTensor& t, bf16** dst) {
  int rc = h->alloc(dst, (size_t)t.numel());
  if (rc) return rc;
  bf16* d = *dst;
  const int rows = (int)t.shape[0], cols = (int)t.shape[1];
  h->params.add(t.name, t.shape, [=](const float* src, hipStream_t s) {
    hipLaunchKernelGGL(pack_transpose_kernel, dim3(cdiv((long)rows * cols, 256)), dim3(256), 0, s, src, d, rows, cols);
    DFOT_CHECK_HIP(hipGetLastError());
    return DFOT_OK;
  });
  return DFOT_OK;
}

// ---- attention-map capture: sizes, buffers ----
size_t dit_cap_map_floats(const dfot_dit_s* h, int form, int batch, int tokens) {
  const DitCfg& c = h->cfg;
  if (c.variant == 3) return (size_t)batch * c.num_col_heads * c.num_row_heads * tokens * tokens;
  if (c.variant == 0 && form == DFOT_ATTN_MAP_FULL) return (size_t)batch * c.num_heads * tokens * h->P * tokens * h->P;
  return (size_t)batch * c.num_heads * tokens * tokens;
}
size_t dit_cap_part_floats(const dfot_dit_s* h, int form, int batch, int tokens) {
  const DitCfg& c = h->cfg;
  if (c.variant == 2) return attention_temporal_map_part_floats(batch, c.num_heads, tokens, h->P);
  if (c.variant == 0 && form == DFOT_ATTN_MAP_FRAME) return attention_map_part_floats(batch, c.num_heads, tokens * h->P, tokens);
  return 0;
}
size_t dit_cap_bytes(const dfot_dit_s* h, int form, size_t nblocks, int batch) {
  return sizeof(float) * (nblocks * dit_cap_map_floats(h, form, batch, h->cfg.max_tokens) + dit_cap_part_floats(h, form, batch, h->cfg.max_tokens));
}
void dit_cap_release(dfot_dit_s* h) {
  for (float* p : h->cap_maps) (void)hipFree(p);
  h->cap_maps.clear();
  if (h->cap_part) (void)hipFree(h->cap_part);
  h->cap_part = nullptr;
  h->cap_bytes = 0;
  h->cap_batch = h->cap_tokens = 0;
}
int dit_cap_alloc(dfot_dit_s* h, int max_batch) {
  dit_cap_release(h);
  const size_t map_bytes = sizeof(float) * dit_cap_map_floats(h, h->cap_form, max_batch, h->cfg.max_tokens);
  const size_t part_bytes = sizeof(float) * dit_cap_part_floats(h, h->cap_form, max_batch, h->cfg.max_tokens);
  for (size_t i = 0; i < h->cap_blocks.size(); ++i) {
    void* p = nullptr;
    DFOT_CHECK_HIP(hipMalloc(&p, map_bytes));
    h->cap_maps.push_back((float*)p);
    h->cap_bytes += map_bytes;
  }
  if (part_bytes) {
    DFOT_CHECK_HIP(hipMalloc((void**)&h->cap_part, part_bytes));
    h->cap_bytes += part_bytes;
  }
  return DFOT_OK;
}
int dit_cap_slot(const dfot_dit_s* h, int block) {
  if (h->cap_form == DFOT_ATTN_MAP_OFF) return -1;
  for (size_t i = 0; i < h->cap_blocks.size(); ++i)
    if (h->cap_blocks[i] == block) return (int)i;
  return -1;
}

int dit_upload(dfot_dit_s* h, float** dst, const std::vector<float>& table) {
  int rc = h->alloc(dst, table.size());
  if (rc) return rc;
  DFOT_CHECK_HIP(hipMemcpy(*dst, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
  return DFOT_OK;
}

int dit_build(dfot_dit_s* h) {
  const DitCfg& c = h->cfg;
  static_cast<DitGeom&>(*h) = dit_geometry(c);
  const int hd = c.hidden_size;
  h->lpad = (c.timesteps + 255) / 256 * 256;
  int rc = 0;
  if ((rc = h->alloc(&h->w_mod, (size_t)h->ldt * hd)) || (rc = h->alloc(&h->b_mod, (size_t)h->ldt))) return rc;
  h->blocks.resize(c.depth);
  if (h->fac) h->fblocks.resize(c.depth);
  if (h->facmat) h->tblocks.resize(c.depth);
  // registration order == the inventory's == the reference module's state_dict order
  for (const DitTensor& t : dit_inventory(c)) {
    DitBlockW* w = t.block < 0 ? nullptr : &(!t.temporal ? h->blocks : h->fac ? h->fblocks : h->tblocks)[t.block];
    if (t.col >= 0) {  // a modulation Linear: rows [col, col + out) of the stacked weight, the same columns of the stacked bias
      if (t.kind == DIT_MOD1_W) w->mod1 = t.col;
      if (t.kind == DIT_MOD2_W) w->mod2 = t.col;
      if (t.shape.size() == 2) h->add_bf16(t.name, (int)t.shape[0], (int)t.shape[1], h->w_mod + t.col * hd);
      else h->add_slice(t.name, t.shape, h->b_mod + t.col);
      continue;
    }
    auto f32 = [&](float** dst) { return h->add_f32(t.name, t.shape, dst); };
    auto linear = [&](bf16** dst) { return h->add_linear(t.name, (int)t.shape[0], (int)t.shape[1], dst); };
    switch (t.kind) {
      case DIT_FZ_FREQS: rc = f32(&h->fz_freqs); break;
      case DIT_FZ_PHASES: rc = f32(&h->fz_phases); break;
      case DIT_T_W1: rc = f32(&h->t_w1); break;
      case DIT_T_B1: rc = f32(&h->t_b1); break;
      case DIT_T_W2: rc = f32(&h->t_w2); break;
      case DIT_T_B2: rc = f32(&h->t_b2); break;
      case DIT_C_W1: rc = f32(&h->c_w1); break;
      case DIT_C_B1: rc = f32(&h->c_b1); break;
      case DIT_C_W2: rc = f32(&h->c_w2); break;
      case DIT_C_B2: rc = f32(&h->c_b2); break;
      case DIT_C_TABLE: rc = f32(&h->c_table); break;
      case DIT_PE_W: rc = f32(&h->pe_w); break;
      case DIT_PE_B: rc = f32(&h->pe_b); break;
      case DIT_DIFF: rc = f32(&h->diff_table); break;
      case DIT_QKV_W: rc = linear(&w->w_qkv); break;
      case DIT_QKV_B: rc = f32(&w->b_qkv); break;
      case DIT_PROJ_W: rc = linear(&w->w_proj); break;
      case DIT_PROJ_B: rc = f32(&w->b_proj); break;
      case DIT_QKV_U: rc = dit_add_transposed(h, t, &w->ut); break;
      case DIT_PROJ_U: rc = dit_add_transposed(h, t, &w->put); break;
      case DIT_QKV_V: rc = dit_add_transposed(h, t, &w->vt); break;
      case DIT_PROJ_V: rc = dit_add_transposed(h, t, &w->pvt); break;
      case DIT_QKV_BIAS: rc = f32(&w->qkv_bias); break;
      case DIT_PROJ_BIAS: rc = f32(&w->proj_bias); break;
      case DIT_FC1_W: rc = linear(&w->w_fc1); break;
      case DIT_FC1_B: rc = f32(&w->b_fc1); break;
      case DIT_FC2_W: rc = linear(&w->w_fc2); break;
      case DIT_FC2_B: rc = f32(&w->b_fc2); break;
      case DIT_FIN_W: rc = f32(&h->fin_w); break;
      case DIT_FIN_B: rc = f32(&h->fin_b); break;
      default: break;  // the modulation kinds: bound above by their column
    }
    if (rc) return rc;
  }

  // derived tables (a fourier_noise model has no finite set of levels: nothing is tabulated, the embedding runs per frame in forward)
  if (!c.fourier_noise) {
    if ((rc = dit_upload(h, &h->freqs, dit_timestep_freqs(c)))) return rc;
    if ((rc = h->alloc(&h->feat, (size_t)h->lpad * c.noise_dim))) return rc;
    if ((rc = h->alloc(&h->thid, (size_t)h->lpad * hd))) return rc;
    if ((rc = h->alloc(&h->emb, (size_t)h->lpad * hd))) return rc;
    const int nflag = h->diffm ? 2 : 1;  // variant 1: the conditioning also depends on the token kind (difference / frame)
    if ((rc = h->alloc(&h->semb, (size_t)nflag * h->lpad * hd))) return rc;
    if ((rc = h->alloc(&h->mod_table, (size_t)nflag * h->lpad * h->ldt))) return rc;
  }
  // positional tables (dit_model.h): sinusoidal_2d at the patch embedding of the factorized variants (+ the temporal table of variant 2,
  // the RoPE-1D of variant 3's matrix attention), RoPE-3D of the full-attention variant
  if (h->facmat || h->fac) {
    if ((rc = dit_upload(h, &h->pos2d, dit_sinusoidal_2d(c, *h)))) return rc;
    if (h->fac && (rc = dit_upload(h, &h->tpos, dit_sinusoidal_1d(c)))) return rc;
    if (c.variant == 3 && c.use_temporal_rope && (rc = dit_upload(h, &h->trope, dit_rope_1d(c)))) return rc;
  } else if ((rc = dit_upload(h, &h->rope_cs, dit_rope_3d(c, *h)))) {
    return rc;
  }
  return DFOT_OK;
}

}  // namespace
}  // namespace dfot

extern "C" {

int dfot_dit_destroy(dfot_dit_t h) {
  if (!h) return DFOT_OK;
  h->free_all();
  dit_cap_release(h);
  for (hipEvent_t e : h->ev_start) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->ev_stop) (void)hipEventDestroy(e);
  delete h;
  return DFOT_OK;
}

static int dit_create_impl(const DitCfg& c, dfot_dit_t* out) {
  DFOT_REQUIRE(c.hidden_size > 0 && c.hidden_size % 64 == 0 && c.hidden_size <= 2048, DFOT_ERR_SHAPE,
               "hidden_size %d must be a multiple of 64, <= 2048", c.hidden_size);
  DFOT_REQUIRE(c.num_heads > 0 && c.hidden_size % c.num_heads == 0, DFOT_ERR_SHAPE, "hidden_size %d not divisible by %d heads",
               c.hidden_size, c.num_heads);
  const int d = c.hidden_size / c.num_heads;
  DFOT_REQUIRE(d % 8 == 0 && d <= 128, DFOT_ERR_SHAPE, "head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(c.patch_size > 0 && c.height % c.patch_size == 0 && c.width % c.patch_size == 0, DFOT_ERR_SHAPE,
               "x_shape %dx%d not divisible by patch %d", c.height, c.width, c.patch_size);
  DFOT_REQUIRE(c.in_channels > 0 && c.in_channels * c.patch_size * c.patch_size <= 256, DFOT_ERR_SHAPE, "patch vector too long");
  DFOT_REQUIRE(c.mlp_hidden >= 0 && c.mlp_hidden % 64 == 0, DFOT_ERR_SHAPE, "mlp_hidden %d must be a multiple of 64", c.mlp_hidden);
  DFOT_REQUIRE(c.noise_dim > 0 && c.noise_dim % 2 == 0 && c.timesteps > 0 && c.max_tokens > 0 && c.depth > 0, DFOT_ERR_SHAPE,
               "bad noise_dim / timesteps / max_tokens / depth");
  DFOT_REQUIRE(c.variant == 0 || c.variant == 1 || c.variant == 2 || c.variant == 3, DFOT_ERR_ARG,
               "variant %d unknown (0 = dit3d full/rope_3d, 1 = difference_dit3d factorized matrix, 2 = dit3d factorized attention, "
               "3 = dit3d factorized matrix)", c.variant);
  if (c.variant == 2) {
    const int P = (c.height / c.patch_size) * (c.width / c.patch_size);
    DFOT_REQUIRE(P % 128 == 0 || P == 64, DFOT_ERR_SHAPE, "factorized attention variant: %d patches per frame must be a multiple of 128, or 64", P);
    DFOT_REQUIRE(P != 64 || c.max_tokens % 2 == 0, DFOT_ERR_SHAPE,
                 "factorized attention variant: max_tokens %d x 64 patches per frame = %d rows per window; the row tiles need a multiple of 128",
                 c.max_tokens, c.max_tokens * 64);
    DFOT_REQUIRE(c.max_tokens <= 32, DFOT_ERR_SHAPE, "factorized attention variant: max_tokens %d exceeds 32", c.max_tokens);
    DFOT_REQUIRE(c.temporal_mlp_hidden >= 0 && c.temporal_mlp_hidden % 64 == 0, DFOT_ERR_SHAPE, "temporal_mlp_hidden %d must be a multiple of 64",
                 c.temporal_mlp_hidden);
  }
  if (c.variant == 1 || c.variant == 3) {  // the models with matrix blocks
    const int P = (c.height / c.patch_size) * (c.width / c.patch_size);
    // 64 patches (attention_seq64.hip runs the per-frame attention): DiT3D's variant 3 only; the difference model keeps its rule
    DFOT_REQUIRE(P % 128 == 0 || (P == 64 && c.variant == 3), DFOT_ERR_SHAPE,
                 "factorized matrix variant: %d patches per frame must be a multiple of 128%s", P, c.variant == 3 ? ", or 64" : "");
    DFOT_REQUIRE(P != 64 || c.max_tokens % 2 == 0, DFOT_ERR_SHAPE,
                 "factorized matrix variant: max_tokens %d x 64 patches per frame = %d rows per window; the row tiles need a multiple of 128",
                 c.max_tokens, c.max_tokens * 64);
    if (c.variant == 3)  // 1 .. 32: the streaming left factors of facmat_narrow.hip; multiples of 64: the factor GEMMs
      DFOT_REQUIRE((c.embed_col_dim >= 1 && c.embed_col_dim <= 32) || (c.embed_col_dim > 0 && c.embed_col_dim % 64 == 0), DFOT_ERR_SHAPE,
                   "embed_col_dim %d must be 1 to 32 (the narrow factor kernels) or a multiple of 64 (the factor GEMMs)", c.embed_col_dim);
    else
      DFOT_REQUIRE(c.embed_col_dim > 0 && c.embed_col_dim % 64 == 0, DFOT_ERR_SHAPE, "embed_col_dim %d must be a multiple of 64", c.embed_col_dim);
    DFOT_REQUIRE(c.num_col_heads > 0 && c.embed_col_dim % c.num_col_heads == 0 && c.num_row_heads > 0 &&
                     c.hidden_size % c.num_row_heads == 0 && (c.hidden_size / c.num_row_heads) % 4 == 0,
                 DFOT_ERR_SHAPE, "matrix attention heads (%d col, %d row) do not divide (%d, %d)", c.num_col_heads, c.num_row_heads,
                 c.embed_col_dim, c.hidden_size);
    DFOT_REQUIRE(c.variant != 1 || (c.max_tokens % 2 == 0 && c.max_tokens <= 32), DFOT_ERR_SHAPE,
                 "max_tokens %d must be even (difference, frame pairs) and <= 32", c.max_tokens);
    DFOT_REQUIRE(c.variant != 3 || c.max_tokens <= 32, DFOT_ERR_SHAPE, "factorized matrix variant: max_tokens %d exceeds 32", c.max_tokens);
    DFOT_REQUIRE(c.temporal_mlp_hidden >= 0 && c.temporal_mlp_hidden % 64 == 0, DFOT_ERR_SHAPE, "temporal_mlp_hidden %d must be a multiple of 64",
                 c.temporal_mlp_hidden);
    DFOT_REQUIRE(c.variant != 3 || c.rope_theta > 0.f || !c.use_temporal_rope, DFOT_ERR_ARG, "rope_theta %g must be positive", (double)c.rope_theta);
  }
  DFOT_REQUIRE(c.cond_type == DFOT_COND_NONE || c.cond_type == DFOT_COND_ACTION || c.cond_type == DFOT_COND_LABEL, DFOT_ERR_ARG,
               "cond_type %d unknown (0 = none, 1 = action, 2 = label)", c.cond_type);
  DFOT_REQUIRE(c.cond_type != DFOT_COND_ACTION || (c.cond_dim > 0 && c.cond_dim <= 1024), DFOT_ERR_SHAPE, "action condition: cond_dim %d must be in [1, 1024]", c.cond_dim);
  DFOT_REQUIRE(c.cond_type != DFOT_COND_LABEL || c.num_classes > 0, DFOT_ERR_SHAPE, "label condition: num_classes %d must be positive", c.num_classes);
  DFOT_REQUIRE(!c.fourier_noise || c.noise_dim <= 2048, DFOT_ERR_SHAPE, "fourier_noise: noise_dim %d exceeds 2048", c.noise_dim);
  auto* h = new dfot_dit_s();
  h->cfg = c;
  int rc = dit_build(h);
  if (rc) {
    dfot_dit_destroy(h);
    return rc;
  }
  *out = h;
  return DFOT_OK;
}

int dfot_dit_create(const dfot_dit_config* cfg, dfot_dit_t* out) {
  DFOT_REQUIRE(cfg && out, DFOT_ERR_ARG, "dfot_dit_create: null argument");
  return dit_create_impl(dit_cfg(*cfg), out);
}

int dfot_dit_create_f(const dfot_dit_config_f* cfg, dfot_dit_t* out) {
  DFOT_REQUIRE(cfg && out, DFOT_ERR_ARG, "dfot_dit_create_f: null argument");
  return dit_create_impl(dit_cfg(cfg->base, cfg->fourier_noise), out);
}

int dfot_dit_num_params(dfot_dit_t h) { return h ? h->params.count() : 0; }
const char* dfot_dit_param_name(dfot_dit_t h, int i) { return h ? h->params.name(i) : nullptr; }
int dfot_dit_param_shape(dfot_dit_t h, int i, int64_t shape[4], int* ndim) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "param_shape: bad argument");
  return h->params.shape(i, shape, ndim);
}

int dfot_dit_load_weight(dfot_dit_t h, const char* name, const float* data, const int64_t* shape, int ndim, void* stream) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "load_weight: null argument");
  int rc = h->params.load(name, data, shape, ndim, (hipStream_t)stream);
  if (!rc) h->finalized = false;
  return rc;
}

int dfot_dit_finalize(dfot_dit_t h, void* stream) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "finalize: null handle");
  int rc = h->params.require_all_loaded();
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const DitCfg& c = h->cfg;
  const int hd = c.hidden_size, L = c.timesteps;
  if (c.fourier_noise) {  // nothing to tabulate; the per-frame modulation GEMM takes 256-row tiles whatever the batch (same bits alone / in a batch)
    h->mod_variant = gemm_pick_variant(A_DENSE, 256, (int)h->ldt, hd, true);
    DFOT_CHECK_HIP(hipStreamSynchronize(s));
    h->finalized = true;
    return DFOT_OK;
  }
  // embedding of every level: features -> Linear -> SiLU -> Linear (emb) ; semb = bf16(SiLU(emb)) feeds every modulation
  hipLaunchKernelGGL(tstep_features_kernel, dim3(cdiv((long)L * c.noise_dim, 256)), dim3(256), 0, s, h->freqs, h->feat, L, c.noise_dim);
  DFOT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rows_linear_kernel<1>, dim3(cdiv(hd, 4), L), dim3(256), 0, s, h->feat, h->t_w1, h->t_b1, h->thid,
                     (bf16*)nullptr, c.noise_dim, hd);
  DFOT_CHECK_HIP(hipGetLastError());
  const int nflag = c.variant == 1 ? 2 : 1;
  DFOT_CHECK_HIP(hipMemsetAsync(h->semb, 0, (size_t)nflag * h->lpad * hd * sizeof(bf16), s));
  hipLaunchKernelGGL(rows_linear_kernel<0>, dim3(cdiv(hd, 4), L), dim3(256), 0, s, h->thid, h->t_w2, h->t_b2, h->emb,
                     c.variant == 1 ? (bf16*)nullptr : h->semb, hd, hd);
  DFOT_CHECK_HIP(hipGetLastError());
  if (c.variant == 1) {  // c = noise-level embedding + diff_embedder(token kind)  (difference_dit3d.py:199-204)
    hipLaunchKernelGGL(add_diff_silu_kernel, dim3(cdiv(2L * L * hd, 256)), dim3(256), 0, s, h->emb, h->diff_table, h->semb, L, h->lpad, hd, 2);
    DFOT_CHECK_HIP(hipGetLastError());
  }
  // mod_table[level][:] = W_mod * SiLU(emb[level]) + b_mod for every modulation of the model
  GemmArgs g;
  g.A = h->semb; g.lda = hd; g.W = h->w_mod; g.M = nflag * h->lpad; g.N = (int)h->ldt; g.K = hd;
  g.bias = h->b_mod; g.out_f32 = h->mod_table; g.ldo = h->ldt;
  h->mod_variant = gemm_pick_variant(A_DENSE, g.M, g.N, g.K, true);
  if ((rc = launch_gemm(A_DENSE, E_F32, h->mod_variant, g, s))) return rc;
  DFOT_CHECK_HIP(hipStreamSynchronize(s));
  h->finalized = true;
  return DFOT_OK;
}

int dfot_dit_reserve(dfot_dit_t h, int max_batch) {
  DFOT_REQUIRE(h && max_batch > 0, DFOT_ERR_ARG, "reserve: bad argument");
  if (max_batch <= h->max_batch) return DFOT_OK;
  if (h->cap_form != DFOT_ATTN_MAP_OFF) {  // refused before anything is freed
    const size_t need = dit_cap_bytes(h, h->cap_form, h->cap_blocks.size(), max_batch);
    DFOT_REQUIRE(need <= h->cap_max_bytes, DFOT_ERR_SHAPE,
                 "reserve: the captured attention maps of %zu blocks need %zu bytes at batch %d x %d tokens, above max_bytes %zu", h->cap_blocks.size(),
                 need, max_batch, h->cfg.max_tokens, h->cap_max_bytes);
  }
  h->free_workspace();
  h->max_batch = 0;
  const DitCfg& c = h->cfg;
  const size_t rows = (size_t)max_batch * c.max_tokens * h->P;
  const size_t qkv = (size_t)max_batch * c.num_heads * c.max_tokens * h->P * h->dstride;
  int rc = 0;
  if ((rc = h->alloc(&h->X, rows * c.hidden_size, true))) return rc;
  if ((rc = h->alloc(&h->A, rows * c.hidden_size, true))) return rc;
  if ((rc = h->alloc(&h->q, qkv, true)) || (rc = h->alloc(&h->k, qkv, true)) || (rc = h->alloc(&h->v, qkv, true))) return rc;
  // pad columns d..dstride of q/k/v are never written by the QKV epilogue: zero them once
  DFOT_CHECK_HIP(hipMemset(h->q, 0, qkv * sizeof(bf16)));
  DFOT_CHECK_HIP(hipMemset(h->k, 0, qkv * sizeof(bf16)));
  DFOT_CHECK_HIP(hipMemset(h->v, 0, qkv * sizeof(bf16)));
  const int hid_cols = c.variant != 0 && c.temporal_mlp_hidden > c.mlp_hidden ? c.temporal_mlp_hidden : c.mlp_hidden;
  if (hid_cols && (rc = h->alloc(&h->hid, rows * hid_cols, true))) return rc;
  if (c.variant == 1) {
    const size_t frames = (size_t)max_batch * c.max_tokens;
    if ((rc = h->alloc(&h->T1, rows * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->W1, frames * c.embed_col_dim * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->W2, frames * c.embed_col_dim * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->Z, frames * c.embed_col_dim * 3 * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->idx, frames, true))) return rc;
  }
  if (c.variant == 3 && c.embed_col_dim <= 32) {
    // narrow column widths (facmat_narrow.hip): no transposes, so T1 holds the expanded frames and W2 is not needed.  The right-factor
    // GEMM runs over frames * E rows rounded up to whole 128-row tiles: W1 and Z are sized to that and zeroed here.  The contract kernel
    // and the attention write the real rows only, so a pad row holds zeros or a real row of an earlier, larger call: finite operands whose
    // products (rows of Z past frames * E) are never read.
    const size_t frames = (size_t)max_batch * c.max_tokens, wrows = (frames * c.embed_col_dim + 127) / 128 * 128;
    if ((rc = h->alloc(&h->T1, frames * h->P * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->W1, wrows * c.hidden_size, true)) || (rc = h->alloc(&h->Z, 3 * wrows * c.hidden_size, true))) return rc;
    DFOT_CHECK_HIP(hipMemset(h->W1, 0, wrows * c.hidden_size * sizeof(bf16)));
    DFOT_CHECK_HIP(hipMemset(h->Z, 0, 3 * wrows * c.hidden_size * sizeof(bf16)));
  } else if (c.variant == 3) {
    // the factor GEMMs of the matrix blocks take whole 128-row tiles: frames * E and frames * hidden rows, both multiples of 64, so an odd
    // frame count runs them on one more frame.  That frame holds the zeros written here or a real frame of an earlier, larger call (the
    // transposes and the attention kernel touch the real frames only): finite operands whose products are never read.
    const size_t frames = (size_t)max_batch * c.max_tokens + 1, fe = frames * c.embed_col_dim * c.hidden_size;
    if ((rc = h->alloc(&h->T1, frames * h->P * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->W1, fe, true)) || (rc = h->alloc(&h->W2, fe, true)) || (rc = h->alloc(&h->Z, 3 * fe, true))) return rc;
    DFOT_CHECK_HIP(hipMemset(h->T1, 0, frames * h->P * c.hidden_size * sizeof(bf16)));
    DFOT_CHECK_HIP(hipMemset(h->W1, 0, fe * sizeof(bf16)));
    DFOT_CHECK_HIP(hipMemset(h->W2, 0, fe * sizeof(bf16)));
    DFOT_CHECK_HIP(hipMemset(h->Z, 0, 3 * fe * sizeof(bf16)));
  }
  if (c.cond_type != DFOT_COND_NONE || c.fourier_noise) {
    const size_t frames = (size_t)max_batch * c.max_tokens;
    if (c.fourier_noise && ((rc = h->alloc(&h->nfeat, frames * c.noise_dim, true)) || (rc = h->alloc(&h->nact, frames * c.hidden_size, true)))) return rc;
    h->fpad = (int)((frames + 255) / 256 * 256);  // whole row tiles of every GEMM form finalize() may have picked
    if ((rc = h->alloc(&h->csemb, (size_t)h->fpad * c.hidden_size, true))) return rc;
    DFOT_CHECK_HIP(hipMemset(h->csemb, 0, (size_t)h->fpad * c.hidden_size * sizeof(bf16)));  // rows past the batch: finite operands
    if ((rc = h->alloc(&h->cmod, (size_t)h->fpad * h->ldt, true))) return rc;
    if ((rc = h->alloc(&h->cemb, frames * c.hidden_size, true))) return rc;
    if ((rc = h->alloc(&h->cidx, frames, true))) return rc;
  }
  if (h->cap_form != DFOT_ATTN_MAP_OFF && (rc = dit_cap_alloc(h, max_batch))) return rc;
  h->max_batch = max_batch;
  return DFOT_OK;
}

size_t dfot_dit_workspace_bytes(dfot_dit_t h) { return h ? h->ws_bytes + h->cap_bytes : 0; }

int dfot_dit_set_option(dfot_dit_t h, const char* key, int value) {
  DFOT_REQUIRE(h && key, DFOT_ERR_ARG, "set_option: null argument");
  if (!strcmp(key, "gemm_variant")) {
    h->gemm_variant = value;
    return DFOT_OK;
  }
  if (!strcmp(key, "front_only")) {
    h->front_only = value != 0;
    return DFOT_OK;
  }
  if (!strcmp(key, "time_attn")) {
    h->time_attn = value > 0;
    h->ev_used = 0;
    while ((int)h->ev_start.size() < value) {
      hipEvent_t a, b;
      DFOT_CHECK_HIP(hipEventCreate(&a));
      DFOT_CHECK_HIP(hipEventCreate(&b));
      h->ev_start.push_back(a);
      h->ev_stop.push_back(b);
    }
    return DFOT_OK;
  }
  set_error("set_option: unknown key '%s'", key);
  return DFOT_ERR_NAME;
}

int dfot_dit_attn_timing(dfot_dit_t h, double* total_ms, int64_t* launches) {
  DFOT_REQUIRE(h && total_ms && launches, DFOT_ERR_ARG, "attn_timing: null argument");
  double tot = 0;
  for (size_t i = 0; i < h->ev_used; ++i) {
    DFOT_CHECK_HIP(hipEventSynchronize(h->ev_stop[i]));
    float ms = 0.f;
    DFOT_CHECK_HIP(hipEventElapsedTime(&ms, h->ev_start[i], h->ev_stop[i]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = (int64_t)h->ev_used;
  h->ev_used = 0;
  return DFOT_OK;
}

}  // extern "C"

// the forward of both entry points; cond / labels == nullptr: the per-level modulation table (no condition)
// flevels: the float levels of a fourier_noise model (noise_levels == nullptr then)
static int dit_forward_impl(dfot_dit_t h, const float* x, const int32_t* noise_levels, const float* cond, const int32_t* labels,
                            const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream, const float* flevels = nullptr) {
  DFOT_REQUIRE(h && x && (noise_levels || flevels) && out, DFOT_ERR_ARG, "forward: null argument");
  DFOT_REQUIRE(!h->cfg.fourier_noise || flevels, DFOT_ERR_ARG,
               "forward: this model embeds float noise levels (fourier_noise); call dfot_dit_forward_f");
  DFOT_REQUIRE(h->cfg.fourier_noise || !flevels, DFOT_ERR_ARG,
               "forward_f: this model indexes integer noise levels (no fourier_noise); call dfot_dit_forward / dfot_dit_forward_cond");
  DFOT_REQUIRE(h->finalized, DFOT_ERR_STATE, "forward: weights not finalized");
  DFOT_REQUIRE(batch > 0 && batch <= h->max_batch, DFOT_ERR_STATE, "forward: batch %d exceeds the reserved %d", batch, h->max_batch);
  const DitCfg& c = h->cfg;
  DFOT_REQUIRE(tokens > 0 && tokens <= c.max_tokens, DFOT_ERR_SHAPE, "forward: %d tokens, max_tokens is %d", tokens, c.max_tokens);
  const int n = tokens * h->P, hd = c.hidden_size;
  DFOT_REQUIRE(n % 128 == 0, DFOT_ERR_SHAPE, "forward: sequence length %d (tokens x patches) must be a multiple of 128", n);
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)batch * n;
  const bool diffm = c.variant == 1, facmat = c.variant == 1 || c.variant == 3, fac = c.variant == 2;
  const int frames = batch * tokens, P = h->P, E = c.embed_col_dim;
  const int gframes = c.variant == 3 ? (frames + 1) & ~1 : frames;  // frames of the matrix blocks' factor GEMMs (see reserve)
  const bool narrow = c.variant == 3 && E <= 32;                    // the left factors are the streaming kernels of facmat_narrow.hip
  DFOT_REQUIRE(!diffm || tokens % 2 == 0, DFOT_ERR_SHAPE, "forward: %d tokens; the difference model takes (difference, frame) pairs", tokens);
  int max_level = c.timesteps - 1;
  const int* lvl = noise_levels;
  const float* table = h->mod_table;
  int rc = 0;
  if (flevels) {
    // continuous diffusion: n = MLP(Fourier features) per frame (two launches); without a condition the second also forms e and SiLU(e)
    FourierEmbedArgs fa;
    fa.levels = flevels; fa.freqs = h->fz_freqs; fa.phases = h->fz_phases;
    fa.w1 = h->t_w1; fa.b1 = h->t_b1; fa.w2 = h->t_w2; fa.b2 = h->t_b2;
    fa.feat_out = h->nfeat; fa.act = h->nact; fa.n_out = h->cemb;
    fa.frames = frames; fa.tokens = tokens; fa.dim = c.noise_dim; fa.hidden = hd;
    if (!(cond || labels)) {
      fa.diff_table = diffm ? h->diff_table : nullptr; fa.semb = h->csemb; fa.idx = h->cidx;
    }
    if ((rc = launch_fourier_embed(fa, s))) return rc;
    h->last_feat_frames = frames;
  }
  if (cond || labels || flevels) {
    // per-frame conditioning: e = noise-level embedding (+ token kind) + condition embedding, then the modulation GEMM over the frames
    // (same tile form as finalize(): a frame without a condition gets the bits of its mod_table row); the blocks index it by frame
    CondEmbedArgs a;
    a.cond = cond; a.labels = labels; a.mask = cond_mask;
    a.w1 = h->c_w1; a.b1 = h->c_b1; a.w2 = h->c_w2; a.b2 = h->c_b2; a.table = h->c_table;
    a.base = flevels ? h->cemb : h->emb; a.levels = flevels ? nullptr : noise_levels; a.max_level = c.timesteps - 1;
    a.diff_table = diffm ? h->diff_table : nullptr;
    a.e_out = h->cemb; a.semb = h->csemb; a.idx = h->cidx;  // (fourier: e overwrites n in place, element by element)
    a.tokens = tokens; a.cond_dim = c.cond_dim; a.hidden = hd; a.table_rows = h->c_rows;
    if ((cond || labels) && (rc = launch_cond_embed(a, frames, s))) return rc;
    GemmArgs g;
    g.A = h->csemb; g.lda = hd; g.W = h->w_mod; g.M = (frames + 255) / 256 * 256; g.N = (int)h->ldt; g.K = hd;
    g.bias = h->b_mod; g.out_f32 = h->cmod; g.ldo = h->ldt;
    if ((rc = launch_gemm(A_DENSE, E_F32, h->mod_variant, g, s))) return rc;
    h->last_cond_frames = frames;
    table = h->cmod;
    lvl = h->cidx;
    max_level = frames - 1;
  } else if (diffm) {  // table row = level + lpad * (token kind)
    hipLaunchKernelGGL(make_index_kernel, dim3(cdiv(frames, 256)), dim3(256), 0, s, noise_levels, h->idx, frames, tokens, max_level, h->lpad);
    DFOT_CHECK_HIP(hipGetLastError());
    lvl = h->idx;
    max_level = 2 * h->lpad - 1;
  }
  if (h->front_only) return DFOT_OK;
  if ((rc = launch_patch_embed(x, h->pe_w, h->pe_b, h->pos2d, h->X, c.in_channels, c.height, c.width, c.patch_size, hd, rows, s))) return rc;
  const float qscale = 1.4426950408889634f / sqrtf((float)h->d);  // attention works in the exp2 domain
  auto ln_mod = [&](long off) -> int {
    return launch_ln_mod(h->X, h->X, h->A, table, lvl, h->ldt, off, hd, P, (int)rows, c.eps, max_level, s);
  };
  auto gated = [&](const bf16* a, int kdim, const bf16* w, const float* bias, int bias_rows, long gate_off) -> int {
    GemmArgs g;  // X <- X + gate * (a W^T + bias), in place
    g.A = a; g.lda = kdim; g.W = w; g.M = (int)rows; g.N = hd; g.K = kdim; g.bias = bias; g.bias_rows = bias_rows;
    g.out_f32 = h->X; g.ldo = hd; g.resid = h->X;
    g.gate = table + gate_off; g.gate_index = lvl; g.ldg = h->ldt; g.gate_rows = P;
    return launch_gemm(A_DENSE, E_F32, h->gemm_variant, g, s);
  };
  auto mlp = [&](long mod2, int hidden_cols, const bf16* w1, const float* b1, const bf16* w2, const float* b2) -> int {
    int r2 = ln_mod(mod2);
    if (r2) return r2;
    GemmArgs g;
    g.A = h->A; g.lda = hd; g.W = w1; g.M = (int)rows; g.N = hidden_cols; g.K = hd; g.bias = b1;
    g.out_bf16 = h->hid; g.ldo = hidden_cols; g.act = 1;
    if ((r2 = launch_gemm(A_DENSE, E_BF16, h->gemm_variant, g, s))) return r2;
    return gated(h->hid, hidden_cols, w2, b2, 0, mod2 + 2 * hd);
  };
  auto transpose = [&](const bf16* src, bf16* dst, int R, int C) -> int {  // per frame [R][C] -> [C][R]
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3(C / 64, R / 64, frames), dim3(256), 0, s, src, dst, R, C);
    DFOT_CHECK_HIP(hipGetLastError());
    return DFOT_OK;
  };
  // attention sequences: the whole video (variant 0) or one frame (variants 1 and 2, per-frame spatial blocks without RoPE)
  const int seq = facmat || fac ? P : n, nseq = facmat || fac ? frames : batch;
  // one DiTBlock: AdaLN -> q|k|v -> attention (over the sequences above, or over the frames of every patch position) -> gated projection -> MLP
  auto dit_block = [&](const DitBlockW& w, int mlp_hidden, bool temporal, int map_slot) -> int {
    int r2 = ln_mod(w.mod1);
    if (r2) return r2;
    {
      GemmArgs g;
      g.A = h->A; g.lda = hd; g.W = w.w_qkv; g.M = (int)rows; g.N = 3 * hd; g.K = hd; g.bias = w.b_qkv;
      g.q = h->q; g.k = h->k; g.v = h->v; g.rope_cs = facmat || fac ? nullptr : h->rope_cs; g.heads = c.num_heads; g.d = h->d;
      g.dstride = h->dstride; g.ntok = seq; g.qscale = qscale;
      if ((r2 = launch_gemm(A_DENSE, E_QKV_DIT, h->gemm_variant, g, s))) return r2;
    }
    const bool timed = h->time_attn && h->ev_used < h->ev_start.size();
    if (timed) DFOT_CHECK_HIP(hipEventRecord(h->ev_start[h->ev_used], s));
    if (temporal)
      r2 = launch_attention_temporal(h->q, h->k, h->v, h->A, hd, batch, tokens, P, c.num_heads, h->d, s);
    else if (seq == 64)  // 64 patches per frame (variants 2 and 3): sequences shorter than launch_attention_padded's 128-row tile
      r2 = launch_attention_seq64(h->q, h->k, h->v, h->A, hd, nseq, c.num_heads, h->d, s);
    else
      r2 = launch_attention_padded(h->q, h->k, h->v, h->A, hd, nseq, c.num_heads, seq, h->d, s);
    if (r2) return r2;
    if (timed) DFOT_CHECK_HIP(hipEventRecord(h->ev_stop[h->ev_used++], s));
    if (map_slot >= 0) {  // capture: the map of the q, k the attention kernel just read
      if (temporal)
        r2 = launch_attention_temporal_map(h->q, h->k, h->cap_maps[map_slot], h->cap_part, batch, tokens, P, c.num_heads, h->d, s);
      else
        r2 = launch_attention_map(h->q, h->k, h->cap_maps[map_slot], h->cap_part, h->cap_form == DFOT_ATTN_MAP_FULL, batch, c.num_heads, n, tokens,
                                  h->d, s);
      if (r2) return r2;
    }
    if ((r2 = gated(h->A, hd, w.w_proj, w.b_proj, 0, w.mod1 + 2 * hd))) return r2;
    return mlp_hidden ? mlp(w.mod2, mlp_hidden, w.w_fc1, w.b_fc1, w.w_fc2, w.b_fc2) : DFOT_OK;
  };
  for (size_t bi = 0; bi < h->blocks.size(); ++bi) {
    const int map_slot = dit_cap_slot(h, (int)bi);  // of the block's frame-mixing attention: the block itself only in variant 0
    if ((rc = dit_block(h->blocks[bi], c.mlp_hidden, false, c.variant == 0 ? map_slot : -1))) return rc;
    if (fac) {
      if (bi == 0) {  // sinusoidal_factorized: the temporal table enters after spatial block 0 (dit_base.py:408-411)
        const long total4 = rows * (hd / 4);
        hipLaunchKernelGGL(add_temporal_pos_kernel, dim3(cdiv(total4, 256)), dim3(256), 0, s, h->X, h->tpos, tokens, P, hd / 4, total4);
        DFOT_CHECK_HIP(hipGetLastError());
      }
      if ((rc = dit_block(h->fblocks[bi], c.temporal_mlp_hidden, true, map_slot))) return rc;
    }
    if (!facmat) continue;

    // ---- MatrixDiTBlock: every frame is one token; qkv = U^T m V + bias, o = softmax(q k^T) v, out = U'^T o V' + bias' ----
    const DitBlockW& t = h->tblocks[bi];
    if ((rc = ln_mod(t.mod1))) return rc;
    if (narrow) {  // left factor in the natural layout: w[frame][e][d] = sum_p U[p][e] m[frame][p][d]  (facmat_narrow.hip)
      if ((rc = launch_facmat_contract(h->A, t.ut, h->W1, frames, P, hd, E, s))) return rc;
    } else {
      if ((rc = transpose(h->A, h->T1, P, hd))) return rc;  // m^T per frame: [hd][P]
      GemmArgs g;  // left factor: w[frame][e][d] = sum_p U[p][e] m[frame][p][d]   (rows (frame, d), K = p, transposed store)
      g.A = h->T1; g.lda = P; g.W = t.ut; g.M = gframes * hd; g.N = E; g.K = P; g.out_bf16 = h->W1; g.ldo = E; g.tr_rows = hd;
      if ((rc = launch_gemm(A_DENSE, E_BF16, h->gemm_variant, g, s))) return rc;
    }
    {
      GemmArgs g;  // right factor + bias[e][k]  (narrow: frames * E rows rounded up to whole tiles, see reserve)
      g.A = h->W1; g.lda = hd; g.W = t.vt; g.M = narrow ? (frames * E + 127) / 128 * 128 : gframes * E; g.N = 3 * hd; g.K = hd;
      g.bias = t.qkv_bias; g.bias_rows = t.qkv_bias ? E : 0;
      g.out_bf16 = h->Z; g.ldo = 3 * hd;
      if ((rc = launch_gemm(A_DENSE, E_BF16, h->gemm_variant, g, s))) return rc;
    }
    {
      const int hn = E / c.num_col_heads, hdr = hd / c.num_row_heads;
      const float mscale = 1.0f / sqrtf((float)hn * (float)hdr);
      if (diffm)
        rc = launch_matrix_attn(h->Z, h->W1, batch, tokens, E, hd, c.num_col_heads, c.num_row_heads, mscale, s);
      else  // FacMatDiT: any 1 <= tokens <= 32, RoPE-1D over the frame axis when the model has one (trope == nullptr: none)
        rc = launch_matrix_attn_rope(h->Z, h->W1, h->trope, batch, tokens, E, hd, c.num_col_heads, c.num_row_heads, mscale, s);
      if (rc) return rc;
      if (!diffm && map_slot >= 0 &&
          (rc = launch_matrix_attn_map(h->Z, h->trope, h->cap_maps[map_slot], batch, tokens, E, hd, c.num_col_heads, c.num_row_heads, mscale, s)))
        return rc;
    }
    if (narrow) {  // left factor of the projection, natural layout: s[frame][p][d] = sum_e U'[e][p] o[frame][e][d]
      if ((rc = launch_facmat_expand(h->W1, t.put, h->T1, frames, P, hd, E, s))) return rc;
    } else {
      if ((rc = transpose(h->W1, h->W2, E, hd))) return rc;  // o^T per frame: [hd][E]
      GemmArgs g;  // left factor of the projection: s[frame][p][d] = sum_e U'[e][p] o[frame][e][d]
      g.A = h->W2; g.lda = E; g.W = t.put; g.M = gframes * hd; g.N = P; g.K = E; g.out_bf16 = h->T1; g.ldo = P; g.tr_rows = hd;
      if ((rc = launch_gemm(A_DENSE, E_BF16, h->gemm_variant, g, s))) return rc;
    }
    if ((rc = gated(h->T1, hd, t.pvt, t.proj_bias, t.proj_bias ? P : 0, t.mod1 + 2 * hd))) return rc;
    if (c.temporal_mlp_hidden && (rc = mlp(t.mod2, c.temporal_mlp_hidden, t.w_fc1, t.b_fc1, t.w_fc2, t.b_fc2))) return rc;
  }
  h->last_rows = (int)rows;
  if (h->cap_form != DFOT_ATTN_MAP_OFF) {
    h->cap_batch = batch;
    h->cap_tokens = tokens;
  }
  return launch_final_layer(h->X, table, lvl, h->ldt, h->mod_final, h->fin_w, h->fin_b, out, hd, P, (int)rows, c.eps,
                            max_level, c.in_channels, c.height, c.width, c.patch_size, s);
}

extern "C" {

int dfot_dit_forward(dfot_dit_t h, const float* x, const int32_t* noise_levels, float* out, int batch, int tokens, void* stream) {
  return dit_forward_impl(h, x, noise_levels, nullptr, nullptr, nullptr, out, batch, tokens, stream);
}

int dfot_dit_forward_cond(dfot_dit_t h, const float* x, const int32_t* noise_levels, const float* cond, const int32_t* labels,
                          const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "forward_cond: null handle");
  const int type = h->cfg.cond_type;
  DFOT_REQUIRE(type != DFOT_COND_NONE, DFOT_ERR_STATE, "forward_cond: this model was built without an external condition embedding");
  DFOT_REQUIRE(type == DFOT_COND_ACTION ? (cond && !labels) : (labels && !cond), DFOT_ERR_ARG,
               "forward_cond: an action model takes `cond` [B,T,cond_dim], a label model takes `labels` [B,T]");
  return dit_forward_impl(h, x, noise_levels, cond, labels, cond_mask, out, batch, tokens, stream);
}

int dfot_dit_forward_f(dfot_dit_t h, const float* x, const float* noise_levels, const float* cond, const int32_t* labels,
                       const uint8_t* cond_mask, float* out, int batch, int tokens, void* stream) {
  DFOT_REQUIRE(h && noise_levels, DFOT_ERR_ARG, "forward_f: null argument");
  const int type = h->cfg.cond_type;
  if (cond || labels) {
    DFOT_REQUIRE(type != DFOT_COND_NONE, DFOT_ERR_STATE, "forward_f: this model was built without an external condition embedding");
    DFOT_REQUIRE(type == DFOT_COND_ACTION ? (cond && !labels) : (labels && !cond), DFOT_ERR_ARG,
                 "forward_f: an action model takes `cond` [B,T,cond_dim], a label model takes `labels` [B,T]");
  } else {
    DFOT_REQUIRE(!cond_mask, DFOT_ERR_ARG, "forward_f: cond_mask without a condition");
  }
  return dit_forward_impl(h, x, nullptr, cond, labels, cond_mask, out, batch, tokens, stream, noise_levels);
}

int dfot_dit_read_tap(dfot_dit_t h, const char* name, float* out, size_t capacity, void* stream) {
  DFOT_REQUIRE(h && name && out, DFOT_ERR_ARG, "read_tap: null argument");
  hipStream_t s = (hipStream_t)stream;
  const float* src = nullptr;
  size_t need = 0;
  if (!strcmp(name, "noise_feat")) {  // Fourier features of every frame of the last dfot_dit_forward_f
    DFOT_REQUIRE(h->last_feat_frames > 0, DFOT_ERR_STATE, "read_tap: no float-level forward has run");
    src = h->nfeat;
    need = (size_t)h->last_feat_frames * h->cfg.noise_dim;
  } else if (!strcmp(name, "emb")) {
    DFOT_REQUIRE(!h->cfg.fourier_noise, DFOT_ERR_ARG, "read_tap: a fourier_noise model keeps no per-level embedding table (tap \"cond_emb\" holds e per frame)");
    DFOT_REQUIRE(h->finalized, DFOT_ERR_STATE, "read_tap: weights not finalized");
    src = h->emb;
    need = (size_t)h->cfg.timesteps * h->cfg.hidden_size;
  } else if (!strcmp(name, "cond_emb")) {  // e = noise-level (+ token-kind) + condition embedding of every frame of the last conditioned forward
    DFOT_REQUIRE(h->last_cond_frames > 0, DFOT_ERR_STATE, "read_tap: no conditioned forward has run");
    src = h->cemb;
    need = (size_t)h->last_cond_frames * h->cfg.hidden_size;
  } else if (!strcmp(name, "stream")) {
    DFOT_REQUIRE(h->last_rows > 0, DFOT_ERR_STATE, "read_tap: no forward has run");
    src = h->X;
    need = (size_t)h->last_rows * h->cfg.hidden_size;
  } else {
    set_error("read_tap: unknown tap '%s'", name);
    return DFOT_ERR_NAME;
  }
  DFOT_REQUIRE(capacity >= need, DFOT_ERR_SHAPE, "read_tap: need %zu floats, got %zu", need, capacity);
  DFOT_CHECK_HIP(hipMemcpyAsync(out, src, need * sizeof(float), hipMemcpyDeviceToDevice, s));
  return DFOT_OK;
}

int dfot_dit_capture_attention(dfot_dit_t h, const int32_t* blocks, int count, int form, size_t max_bytes) {
  DFOT_REQUIRE(h, DFOT_ERR_ARG, "capture_attention: null handle");
  if (form == DFOT_ATTN_MAP_OFF) {
    DFOT_CHECK_HIP(hipDeviceSynchronize());  // a forward that writes the buffers may still be running
    dit_cap_release(h);
    h->cap_form = DFOT_ATTN_MAP_OFF;
    h->cap_blocks.clear();
    return DFOT_OK;
  }
  const DitCfg& c = h->cfg;
  DFOT_REQUIRE(form == DFOT_ATTN_MAP_FRAME || form == DFOT_ATTN_MAP_FULL, DFOT_ERR_ARG, "capture_attention: form %d unknown (-1 = off, 0 = frame, 1 = full)",
               form);
  DFOT_REQUIRE(c.variant != 1, DFOT_ERR_ARG, "capture_attention: the difference model (variant 1, difference_dit3d) is not supported");
  DFOT_REQUIRE(!(c.variant == 2 && form == DFOT_ATTN_MAP_FULL), DFOT_ERR_ARG,
               "capture_attention: form 'full' on the factorized attention variant: a temporal block has one T x T map per patch position and only "
               "their mean, the frame map, is formed");
  if (c.variant == 0)
    DFOT_REQUIRE(h->P % 64 == 0 && c.max_tokens <= 32, DFOT_ERR_SHAPE,
                 "capture_attention: the map kernel needs patches per frame %% 64 == 0 and max_tokens <= 32 (have %d patches, max_tokens %d)", h->P,
                 c.max_tokens);
  DFOT_REQUIRE(count >= 0 && (blocks || count == 0), DFOT_ERR_ARG, "capture_attention: %d blocks without a list", count);
  std::vector<int> sel;
  if (!blocks) {
    for (int i = 0; i < c.depth; ++i) sel.push_back(i);
  } else {
    for (int i = 0; i < count; ++i) {
      DFOT_REQUIRE(blocks[i] >= 0 && blocks[i] < c.depth, DFOT_ERR_ARG, "capture_attention: block index %d outside 0 .. %d", blocks[i], c.depth - 1);
      DFOT_REQUIRE(i == 0 || blocks[i] > blocks[i - 1], DFOT_ERR_ARG, "capture_attention: block indices must ascend (%d after %d)", blocks[i],
                   blocks[i - 1]);
      sel.push_back(blocks[i]);
    }
  }
  const size_t cap = max_bytes ? max_bytes : (size_t)1 << 30;
  const int at_batch = h->max_batch > 0 ? h->max_batch : 1;
  const size_t need = dit_cap_bytes(h, form, sel.size(), at_batch);
  DFOT_REQUIRE(need <= cap, DFOT_ERR_SHAPE, "capture_attention: the %s maps of %zu blocks need %zu bytes at batch %d x %d tokens, above max_bytes %zu",
               form == DFOT_ATTN_MAP_FULL ? "full" : "frame", sel.size(), need, at_batch, c.max_tokens, cap);
  DFOT_CHECK_HIP(hipDeviceSynchronize());
  dit_cap_release(h);
  h->cap_form = form;
  h->cap_blocks = sel;
  h->cap_max_bytes = cap;
  if (h->max_batch > 0) {
    int rc = dit_cap_alloc(h, h->max_batch);
    if (rc) {
      dit_cap_release(h);
      h->cap_form = DFOT_ATTN_MAP_OFF;
      h->cap_blocks.clear();
      return rc;
    }
  }
  return DFOT_OK;
}

int dfot_dit_attention_map_shape(dfot_dit_t h, int slot, int64_t shape[5], int* ndim) {
  DFOT_REQUIRE(h && shape && ndim, DFOT_ERR_ARG, "attention_map_shape: null argument");
  DFOT_REQUIRE(h->cap_form != DFOT_ATTN_MAP_OFF, DFOT_ERR_STATE, "attention_map_shape: attention capture is off");
  DFOT_REQUIRE(slot >= 0 && slot < (int)h->cap_blocks.size(), DFOT_ERR_ARG, "attention_map_shape: slot %d of %zu captured blocks", slot, h->cap_blocks.size());
  DFOT_REQUIRE(h->cap_batch > 0, DFOT_ERR_STATE, "attention_map_shape: no forward has run with the capture on");
  const DitCfg& c = h->cfg;
  const int64_t t = h->cap_tokens;
  int k = 0;
  shape[k++] = h->cap_batch;
  if (c.variant == 3) {
    shape[k++] = c.num_col_heads;
    shape[k++] = c.num_row_heads;
  } else {
    shape[k++] = c.num_heads;
  }
  const int64_t side = c.variant == 0 && h->cap_form == DFOT_ATTN_MAP_FULL ? t * h->P : t;
  shape[k++] = side;
  shape[k++] = side;
  *ndim = k;
  return DFOT_OK;
}

int dfot_dit_read_attention_map(dfot_dit_t h, int slot, float* out, size_t capacity, void* stream) {
  DFOT_REQUIRE(h && out, DFOT_ERR_ARG, "read_attention_map: null argument");
  DFOT_REQUIRE(h->cap_form != DFOT_ATTN_MAP_OFF, DFOT_ERR_STATE, "read_attention_map: attention capture is off");
  DFOT_REQUIRE(slot >= 0 && slot < (int)h->cap_blocks.size(), DFOT_ERR_ARG, "read_attention_map: slot %d of %zu captured blocks", slot, h->cap_blocks.size());
  DFOT_REQUIRE(h->cap_batch > 0 && slot < (int)h->cap_maps.size(), DFOT_ERR_STATE, "read_attention_map: no forward has run with the capture on");
  const size_t need = dit_cap_map_floats(h, h->cap_form, h->cap_batch, h->cap_tokens);
  DFOT_REQUIRE(capacity >= need, DFOT_ERR_SHAPE, "read_attention_map: need %zu floats, got %zu", need, capacity);
  DFOT_CHECK_HIP(hipMemcpyAsync(out, h->cap_maps[slot], need * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DFOT_OK;
}

// test entry of the training path: forward (o, lse) + backward of one attention call; temporaries are allocated here
int dfot_op_attention_bwd(const void* q, const void* k, const void* v, const void* d_o, void* o, int ldo, void* dq, void* dk, void* dv,
                          int batch, int heads, int n, int d, void* stream) {
  DFOT_REQUIRE(q && k && v && d_o && o && dq && dk && dv, DFOT_ERR_ARG, "attention_bwd: null argument");
  // the backward's shape rules (narrower than the forward's) are checked before the forward: nothing runs on a refused call
  if (int rc0 = attention_bwd_shape_check(n, d, ldo)) return rc0;
  hipStream_t s = (hipStream_t)stream;
  const size_t bhn = (size_t)batch * heads * n;
  float *lse = nullptr, *delta = nullptr;
  DFOT_CHECK_HIP(hipMalloc(&lse, bhn * sizeof(float)));
  DFOT_CHECK_HIP(hipMalloc(&delta, bhn * sizeof(float)));
  int rc = launch_attention_padded((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, ldo, batch, heads, n, d, s, lse);
  if (!rc) rc = launch_attention_bwd_delta((const bf16*)o, (const bf16*)d_o, ldo, delta, batch, heads, n, d, s);
  if (!rc) rc = launch_attention_bwd((const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, ldo, lse, delta, (bf16*)dq, (bf16*)dk,
                                     (bf16*)dv, batch, heads, n, d, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(lse); (void)hipFree(delta);
  return rc;
}

int dfot_op_matrix_attention(const void* z, void* o, int batch, int L, int E, int h, int cc, int rr, float scale, void* stream) {
  DFOT_REQUIRE(z && o && batch > 0 && E > 0 && h > 0 && cc > 0 && rr > 0 && E % cc == 0 && h % rr == 0 && (h / rr) % 4 == 0, DFOT_ERR_SHAPE,
               "matrix attention: batch %d, E %d, h %d, heads (%d, %d)", batch, E, h, cc, rr);
  return launch_matrix_attn((const bf16*)z, (bf16*)o, batch, L, E, h, cc, rr, scale, (hipStream_t)stream);
}

int dfot_op_attention_padded(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int heads, int n, int d,
                             void* stream) {
  return launch_attention_padded((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, ldo, batch, heads, n, d, (hipStream_t)stream);
}

static int op_final_layer(const float* x, const float* table, const int32_t* levels, int64_t ldt, int64_t off, const float* w, const float* b,
                          float* out, int hidden, int rows_per_frame, int rows, float eps, int max_level, int c, int hh, int ww, int patch,
                          int form, int chunk, void* stream) {
  DFOT_REQUIRE(x && table && levels && w && b && out, DFOT_ERR_ARG, "final layer: null argument");
  DFOT_REQUIRE(c > 0 && patch > 0 && hh > 0 && ww > 0 && hh % patch == 0 && ww % patch == 0 && rows_per_frame == (hh / patch) * (ww / patch) &&
                   rows > 0 && rows % rows_per_frame == 0,
               DFOT_ERR_SHAPE, "final layer: %d rows of %d per frame for %d x %d frames in patches of %d", rows, rows_per_frame, hh, ww, patch);
  DFOT_REQUIRE((long)c * patch * patch <= 256, DFOT_ERR_SHAPE, "patch vector too long");
  DFOT_REQUIRE(hidden > 0 && hidden <= 2048 && max_level >= 0 && off >= 0 && ldt >= off + 2L * hidden, DFOT_ERR_ARG,
               "final layer: hidden %d, table row of %ld with (shift | scale) at %ld, max_level %d", hidden, (long)ldt, (long)off, max_level);
  return launch_final_layer(x, table, levels, ldt, off, w, b, out, hidden, rows_per_frame, rows, eps, max_level, c, hh, ww, patch,
                            (hipStream_t)stream, form, chunk);
}
int dfot_op_dit_final_layer(const float* x, const float* table, const int32_t* levels, int64_t ldt, int64_t off, const float* w, const float* b,
                            float* out, int hidden, int rows_per_frame, int rows, float eps, int max_level, int c, int h, int width, int patch,
                            int form, void* stream) {
  return op_final_layer(x, table, levels, ldt, off, w, b, out, hidden, rows_per_frame, rows, eps, max_level, c, h, width, patch, form, 0, stream);
}
int dfot_op_dit_final_layer_chunked(const float* x, const float* table, const int32_t* levels, int64_t ldt, int64_t off, const float* w,
                                    const float* b, float* out, int hidden, int rows_per_frame, int rows, float eps, int max_level, int c, int h,
                                    int width, int patch, int chunk, void* stream) {
  DFOT_REQUIRE(chunk > 0, DFOT_ERR_ARG, "final layer: chunk of %d output rows", chunk);
  return op_final_layer(x, table, levels, ldt, off, w, b, out, hidden, rows_per_frame, rows, eps, max_level, c, h, width, patch, 2, chunk, stream);
}

// ---- single launches of the DiT blocks (test entries: each runs the launcher the engines call, on caller-provided buffers) ----
int dfot_op_dit_ln_mod(const float* xin, float* xout, void* obf, const float* table, const int32_t* levels, int64_t ldt, int64_t off, int hidden,
                       int rows_per_frame, int rows, float eps, int max_level, void* stream) {
  DFOT_REQUIRE(xin && xout && obf && table && levels, DFOT_ERR_ARG, "ln_mod: null argument");
  DFOT_REQUIRE(hidden > 0 && rows > 0 && rows_per_frame > 0 && rows % rows_per_frame == 0, DFOT_ERR_SHAPE, "ln_mod: %d rows of %d per frame, hidden %d",
               rows, rows_per_frame, hidden);
  DFOT_REQUIRE(max_level >= 0 && off >= 0 && off % 4 == 0 && ldt % 4 == 0 && ldt >= off + 2L * hidden, DFOT_ERR_ARG,
               "ln_mod: table row of %ld with (shift | scale) at %ld (multiples of 4), max_level %d", (long)ldt, (long)off, max_level);
  return launch_ln_mod(xin, xout, (bf16*)obf, table, levels, ldt, off, hidden, rows_per_frame, rows, eps, max_level, (hipStream_t)stream);
}

// c, h, width, patch of a patch embedding and its row count: the checks of the three patch-embedding entries and of the final gather
static int op_patch_geometry(const char* what, int c, int hh, int ww, int patch, int hidden, int64_t rows) {
  DFOT_REQUIRE(c > 0 && patch > 0 && hh > 0 && ww > 0 && hh % patch == 0 && ww % patch == 0 && hidden > 0, DFOT_ERR_SHAPE,
               "%s: %d channels, %d x %d frames in patches of %d, hidden %d", what, c, hh, ww, patch, hidden);
  DFOT_REQUIRE((long)c * patch * patch <= 256, DFOT_ERR_SHAPE, "%s: patch vector too long (patch_size^2 * channels = %ld, at most 256)", what,
               (long)c * patch * patch);
  DFOT_REQUIRE(rows > 0 && rows % ((hh / patch) * (ww / patch)) == 0 && rows * (long)hidden < (1L << 31) && rows * 256 < (1L << 31), DFOT_ERR_SHAPE,
               "%s: %ld rows are no whole number of %d-patch frames (or too many)", what, (long)rows, (hh / patch) * (ww / patch));
  return DFOT_OK;
}

int dfot_op_dit_patch_embed(const float* x, const float* w, const float* b, const float* pos, float* out, int c, int h, int width, int patch,
                            int hidden, int64_t rows, void* stream) {
  DFOT_REQUIRE(x && w && b && out, DFOT_ERR_ARG, "patch_embed: null argument");
  if (int rc = op_patch_geometry("patch_embed", c, h, width, patch, hidden, rows)) return rc;
  return launch_patch_embed(x, w, b, pos, out, c, h, width, patch, hidden, (long)rows, (hipStream_t)stream);
}

}  // extern "C"

#include "dit_train.inl"
#include "dit1d_train.inl"
#include "uvit_train.inl"
