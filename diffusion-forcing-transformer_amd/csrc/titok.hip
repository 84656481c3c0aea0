// TiTok-KL decoder pieces (algorithms/vae/tiktok_kl/{titok_kl,blocks_kl}.py): the ViT over [cls | grid^2 mask tokens | 32 latent tokens]
// that turns the 1-D token latents of the taichi recipes into the pixel decoder's input.  Its GEMMs, the channel softmax and the whole
// pixel decoder (maskgit_vqgan.Decoder) are ops of gemm.hip / vae.hip / image_vae.hip; this file adds what had no op:
//   dfot_op_mha_packed        nn.MultiheadAttention's core on the packed in-projection output qkv bf16 [rows][q | k | v], heads in adjacent
//                             64-column groups, for RAGGED sequences: `seqs` sequences of `len` rows back to back, any 1 <= len <= 4160
//                             (49 / 97 / 289 / 1057 tokens for 64^2 ... 512^2 frames), so sequences start in the middle of a tile and end
//                             in a partial one.  A workgroup of 2 waves owns 64 query rows (32 per wave) of one (sequence, head) and
//                             streams that head's keys in blocks of 64 through LDS (K and V tiles [64][64], the AttnCfg<64> image of
//                             attention_common.h, global -> registers -> LDS, two stages):
//                               S^T (64 keys x 32 q) = K Q^T                      2 x 4 mfma_f32_32x32x16_bf16, Q fragments in registers
//                               keys >= len are set to -inf BY SELECT, the running row max / sum are updated (fp32, exp2 domain with the
//                               log2(e) / 8 scale folded in HERE, not into the weights), O^T is rescaled,
//                               O^T (64 channels x 32 q) += V^T P^T               2 x 4 MFMAs, P rounded to bf16, V^T by transposed LDS reads
//                             Rows >= len of a K / V tile are staged as ZEROS and never loaded, query rows >= len are neither loaded nor
//                             stored: rows the sequence does not own (the next sequence, the rows that pad `rows` to a GEMM tile, memory
//                             past the buffer) cannot reach a result, whatever they hold.  The summation order depends on (len, heads)
//                             only, so a sequence's bits do not depend on the launch it is part of.
//   dfot_op_layernorm         nn.LayerNorm (affine, eps argument) of fp32 rows -> bf16 and / or fp32 rows; one wave per row, two passes in
//                             registers.  Gather form: output row r reads source row (r / take) * seq_len + first + r % take (ln_post reads
//                             rows 1 .. grid^2 of every sequence and writes the compact GEMM operand).
//   dfot_op_bias_act_bf16     fp32 GEMM output + bias -> GELU (exact erf form, nn.GELU()) or tanh -> bf16
//   dfot_op_titok_tokens      F.normalize(z, dim=1), decoder_embed (K = token_size: VALU), the positional adds, the cls / mask rows and
//                             ln_pre in one launch -> the fp32 residual stream
// and for the encoder half (the same blocks over [cls | grid^2 patches | 32 latent tokens]):
//   dfot_op_titok_patch_rows  frames fp32 (F, 3, S, S) -> the bf16 A operand [F * grid^2][768] of the patch-embedding GEMM
//   dfot_op_titok_enc_tokens  cls / patch rows + positional_embedding, latent_tokens + their positional embedding, ln_pre in one launch
//   dfot_op_titok_moments     conv_out on the reference's reshape of the ln_post rows (a reinterpretation of each frame's block) -> the
//                             moments in the layout dfot_op_vae_posterior reads, all fp32
#include <math.h>

#include "attention_common.h"
#include "common.h"
#include "dfot_hip.h"

namespace dfot {
namespace {

constexpr int MHA_WAVES = 2;                 // waves per workgroup, 32 query rows each
constexpr int MHA_QB = MHA_WAVES * 32;       // query rows per workgroup
constexpr int MHA_THREADS = MHA_WAVES * 64;
constexpr int MHA_MAX_LEN = 4160;            // 1 + 64^2 + 32 = 4129 tokens of a 1024^2 frame fit

__global__ __launch_bounds__(MHA_THREADS) void mha_packed_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o, long ld, long ldo, int len,
                                                                 int heads, int nqb, float scale2) {
  using Cfg = AttnCfg<64>;
  constexpr int PER = 64 * 8 / MHA_THREADS;  // 16-byte chunks each thread stages per [64][64] tile
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * Cfg::TILE];  // [2 stages][K tile | V tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int qb = blockIdx.x % nqb;
  const int head = (blockIdx.x / nqb) % heads;
  const long seq = blockIdx.x / ((long)nqb * heads);
  const bf16* base = qkv + seq * len * ld + head * 64;        // q of row 0 of this sequence; k at + heads * 64, v at + 2 * heads * 64
  const bf16* kbase = base + heads * 64;
  const bf16* vbase = base + 2 * heads * 64;
  const int qrow = qb * MHA_QB + wave * 32 + lq;               // this lane's query row inside the sequence
  const bool qok = qrow < len;
  const int nkb = (len + 63) >> 6;

  bf16x8 zero8;
#pragma unroll
  for (int j = 0; j < 8; ++j) zero8[j] = f2bf(0.f);

  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = qok ? *reinterpret_cast<const bf16x8*>(base + (long)qrow * ld + ks * 16 + lh * 8) : zero8;

  bf16x8 sk[PER], sv[PER];
  auto load_block = [&](int b) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + MHA_THREADS * j;
      const int row = b * 64 + (e >> 3);
      const bool ok = row < len;
      sk[j] = ok ? *reinterpret_cast<const bf16x8*>(kbase + (long)row * ld + (e & 7) * 8) : zero8;
      sv[j] = ok ? *reinterpret_cast<const bf16x8*>(vbase + (long)row * ld + (e & 7) * 8) : zero8;
    }
  };
  auto store_block = [&](int b) {
    char* dk = smem + (b & 1) * 2 * Cfg::TILE;
    char* dv = dk + Cfg::TILE;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + MHA_THREADS * j;
      const int row = e >> 3, c = e & 7;
      *reinterpret_cast<bf16x8*>(dk + row * Cfg::ROWB + Cfg::swz_k(row, c) * 16) = sk[j];
      *reinterpret_cast<bf16x8*>(dv + row * Cfg::ROWB + Cfg::swz_v(row, c) * 16) = sv[j];
    }
  };

  f32x16 oacc[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
  float m = -INFINITY, l = 0.f;

  load_block(0);
  store_block(0);
  __syncthreads();
  for (int b = 0; b < nkb; ++b) {
    const char* tk = smem + (b & 1) * 2 * Cfg::TILE;
    const char* tv = tk + Cfg::TILE;
    if (b + 1 < nkb) load_block(b + 1);

    // ---- S^T = K Q^T: sacc[kt][r] is key b*64 + kt*32 + (r&3) + 8*(r>>2) + 4*lh against query lq ----
    f32x16 sacc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.f;
      const int row = kt * 32 + lq;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(tk + row * Cfg::ROWB + Cfg::swz_k(row, ks * 2 + lh) * 16);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc[kt], 0, 0, 0);
      }
    }
    // ---- ragged tail: keys past len are masked by select; block 0 always holds key 0, so the running max is finite from there on ----
    float bm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = b * 64 + kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        sacc[kt][r] = key < len ? sacc[kt][r] : -INFINITY;
        bm = fmaxf(bm, sacc[kt][r]);
      }
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float mn = fmaxf(m, bm);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * scale2);   // first block: exp2(-inf) = 0
    float rs = 0.f;
    bf16x8 pf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f((sacc[kt][8 * s + j] - mn) * scale2);
          rs += p;
          pf[kt][s][j] = f2bf(p);
        }
    l = l * alpha + (rs + __shfl_xor(rs, 32));
    m = mn;
    // ---- O^T = alpha O^T + V^T P^T ----
#pragma unroll
    for (int dvt = 0; dvt < 2; ++dvt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dvt][r] *= alpha;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_v<64>(tv, dvt, kt, s, lane), pf[kt][s], oacc[dvt], 0, 0, 0);
    }
    if (b + 1 < nkb) store_block(b + 1);
    __syncthreads();
  }

  // lane holds O[qrow][32 dvt + 8 g + 4 lh + {0..3}] in oacc[dvt][4 g .. 4 g + 3]
  if (qok) {
    const float inv = 1.0f / l;
    bf16* orow = o + (seq * len + qrow) * ldo + head * 64;
#pragma unroll
    for (int dvt = 0; dvt < 2; ++dvt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 o4;
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = f2bf(oacc[dvt][4 * g4 + j] * inv);
        *reinterpret_cast<bf16x4*>(orow + dvt * 32 + 8 * g4 + 4 * lh) = o4;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One wave per row of C = 256 n4 channels (n4 <= 4): lane holds the float4 at columns 4 (lane + 64 i).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ void ln_row(f32x4 (&v)[4], int n4, int lane, int c, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                       bf16* out_bf, float* out_f32) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < n4) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) / (float)c;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < n4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[i][j] - mean;
        q += d * d;
      }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)c + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < n4) {
      const int col = 4 * (lane + 64 * i);
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col), bt = *reinterpret_cast<const f32x4*>(beta + col);
      f32x4 y;
      bf16x4 yb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        y[j] = (v[i][j] - mean) * rstd * g[j] + bt[j];
        yb[j] = f2bf(y[j]);
      }
      if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + col) = y;
      if (out_bf) *reinterpret_cast<bf16x4*>(out_bf + col) = yb;
    }
}

__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, bf16* __restrict__ out_bf, float* __restrict__ out_f32, long rows, int c, int seq_len,
                                                        int first, int take) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, n4 = c >> 8;
  const long src = seq_len ? (row / take) * seq_len + first + row % take : row;
  f32x4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < n4) v[i] = *reinterpret_cast<const f32x4*>(x + src * c + 4 * (lane + 64 * i));
  ln_row(v, n4, lane, c, eps, gamma, beta, out_bf ? out_bf + row * c : nullptr, out_f32 ? out_f32 + row * c : nullptr);
}

__global__ __launch_bounds__(256) void bias_act_kernel(const float* __restrict__ x, long ld, const float* __restrict__ bias, bf16* __restrict__ out,
                                                       long total4, int n4, int act) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total4) return;
  const long row = idx / n4;
  const int col = (int)(idx - row * n4) * 4;
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + row * ld + col);
  const f32x4 b = *reinterpret_cast<const f32x4*>(bias + col);
  bf16x4 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float t = v[j] + b[j];
    y[j] = f2bf(act == 0 ? 0.5f * t * (1.0f + erff(t * 0.70710678118654752f)) : tanhf(t));
  }
  *reinterpret_cast<bf16x4*>(out + row * (long)n4 * 4 + col) = y;
}

constexpr int TOK_MAX_TS = 64;  // token_size (latent channels): the K of the VALU embed

__global__ __launch_bounds__(256) void titok_tokens_kernel(const float* __restrict__ z, const float* __restrict__ ew, const float* __restrict__ eb,
                                                           const float* __restrict__ lpos, const float* __restrict__ cls, const float* __restrict__ mask,
                                                           const float* __restrict__ pos, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ out, long rows, int grid2, int nlat, int ts, int c, int l2norm) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, n4 = c >> 8;
  const int len = 1 + grid2 + nlat;
  const long f = row / len;
  const int i = (int)(row - f * len);
  f32x4 v[4];
  if (i <= grid2) {       // [cls | mask tokens] + positional_embedding[i]
    const float* tok = i == 0 ? cls : mask;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n4) {
        const int col = 4 * (lane + 64 * k);
        v[k] = *reinterpret_cast<const f32x4*>(tok + col) + *reinterpret_cast<const f32x4*>(pos + (long)i * c + col);
      }
  } else {                // decoder_embed(normalize(z[f, :, t])) + latent_token_positional_embedding[t]
    const int t = i - 1 - grid2;
    const float* zf = z + f * ts * nlat + t;   // z (F, ts, 1, nlat): channel stride nlat
    float ss = 0.f;
    for (int k = 0; k < ts; ++k) ss += zf[(long)k * nlat] * zf[(long)k * nlat];
    const float inv = l2norm ? 1.0f / fmaxf(sqrtf(ss), 1e-12f) : 1.0f;   // F.normalize: x / max(||x||, 1e-12)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n4) {
        const int col = 4 * (lane + 64 * k);
        f32x4 a = *reinterpret_cast<const f32x4*>(eb + col);
        for (int cc = 0; cc < ts; ++cc) {
          const float zn = zf[(long)cc * nlat] * inv;
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += ew[(long)(col + j) * ts + cc] * zn;
        }
        v[k] = a + *reinterpret_cast<const f32x4*>(lpos + (long)t * c + col);
      }
  }
  ln_row(v, n4, lane, c, eps, gamma, beta, nullptr, out + row * c);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Encoder front and back (blocks_kl.py:140-166).
// The A operand of the patch-embedding GEMM.  One thread per 8 output elements, in destination order: a wave writes 1024 contiguous
// bytes and reads the 16-pixel runs behind them (64 contiguous bytes each, two lanes per run).
__global__ __launch_bounds__(256) void titok_patch_rows_kernel(const float* __restrict__ frames, bf16* __restrict__ rows, long total8, int s, int g) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const long row = idx / 96;                       // 768 / 8 chunks per row
  const int k8 = (int)(idx - row * 96);
  const int c = k8 >> 5, dy = (k8 >> 1) & 15, half = k8 & 1;
  const int g2 = g * g;
  const long f = row / g2;
  const int p = (int)(row - f * g2);
  const int py = p / g, px = p - py * g;
  const float* src = frames + ((f * 3 + c) * s + 16 * py + dy) * (long)s + 16 * px + 8 * half;
  const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = f2bf(a[j]);
    o[4 + j] = f2bf(b[j]);
  }
  *reinterpret_cast<bf16x8*>(rows + row * 768 + k8 * 8) = o;
}

__global__ __launch_bounds__(256) void titok_enc_tokens_kernel(const float* __restrict__ patches, long ldp, const float* __restrict__ cls,
                                                               const float* __restrict__ pos, const float* __restrict__ lat, const float* __restrict__ lpos,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               float* __restrict__ out, long rows, int grid2, int nlat, int c) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, n4 = c >> 8;
  const int len = 1 + grid2 + nlat;
  const long f = row / len;
  const int i = (int)(row - f * len);
  // [cls | patch_embed(x)] + positional_embedding[i], then latent_tokens[t] + latent_token_positional_embedding[t]
  const float* a = i == 0 ? cls : i <= grid2 ? patches + (f * grid2 + i - 1) * ldp : lat + (long)(i - 1 - grid2) * c;
  const float* b = i <= grid2 ? pos + (long)i * c : lpos + (long)(i - 1 - grid2) * c;
  f32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n4) {
      const int col = 4 * (lane + 64 * k);
      v[k] = *reinterpret_cast<const f32x4*>(a + col) + *reinterpret_cast<const f32x4*>(b + col);
    }
  ln_row(v, n4, lane, c, eps, gamma, beta, nullptr, out + row * c);
}

// conv_out on the reference's reshape(batch, width, num_latent, 1) of the contiguous (batch, num_latent, width) ln_post rows: a
// REINTERPRETATION, not a transpose -- "channel" ch at position n is flat element ch * nlat + n of the frame's block.  A workgroup owns
// one frame and two output channels.  Thread e < slices * nlat (slices = 256 / nlat) is position n = e % nlat of slice e / nlat and sums
// the channels ch = slice, slice + slices, ...: in step k the active threads read the flat elements k * slices * nlat + e, contiguous.
// The slices' partial sums are added in slice order: one summation order per (nlat, channels), all fp32.
__global__ __launch_bounds__(256) void titok_moments_kernel(const float* __restrict__ t, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out, long ldo, int nlat, int c, int pairs) {
  __shared__ float part[2][256];
  const int e = threadIdx.x;
  const long f = blockIdx.x / pairs;
  const int o = 2 * (int)(blockIdx.x - f * pairs);
  const int slices = 256 / nlat;
  const int slice = e / nlat, n = e - slice * nlat;
  const float* tf = t + f * (long)nlat * c;
  const float* w0 = w + (long)o * c;
  const float* w1 = w0 + c;
  float a0 = 0.f, a1 = 0.f;
  if (slice < slices)
    for (int ch = slice; ch < c; ch += slices) {
      const float x = tf[(long)ch * nlat + n];
      a0 = fmaf(w0[ch], x, a0);
      a1 = fmaf(w1[ch], x, a1);
    }
  part[0][e] = a0;
  part[1][e] = a1;
  __syncthreads();
  if (e < 2 * nlat) {
    const int j = e / nlat, m = e - j * nlat;
    float s = bias[o + j];
    for (int sl = 0; sl < slices; ++sl) s += part[j][sl * nlat + m];
    out[(f * nlat + m) * ldo + o + j] = s;
  }
}

bool width_ok(int c) { return c == 512 || c == 768 || c == 1024; }

}  // namespace
}  // namespace dfot

extern "C" {
using namespace dfot;

int dfot_op_mha_packed_max_len(void) { return MHA_MAX_LEN; }

int dfot_op_mha_packed(const void* qkv, int64_t ld, void* o, int seqs, int len, int heads, void* stream) {
  DFOT_REQUIRE(qkv && o && qkv != o, DFOT_ERR_ARG, "op_mha_packed: null or aliased argument");
  DFOT_REQUIRE(seqs > 0 && len >= 1 && len <= MHA_MAX_LEN && heads >= 1 && heads <= 64 && ld >= 3L * heads * 64 && ld % 8 == 0, DFOT_ERR_SHAPE,
               "op_mha_packed: seqs=%d sequences of len=%d (1 .. %d) with heads=%d (1 .. 64) of 64 channels, row stride ld=%ld (>= 3 * heads * 64 = %ld, a "
               "multiple of 8)", seqs, len, MHA_MAX_LEN, heads, (long)ld, 3L * heads * 64);
  const int nqb = cdiv(len, MHA_QB);
  const long blocks = (long)seqs * heads * nqb;
  DFOT_REQUIRE(blocks < (1L << 31) && (long)seqs * len * ld < (1L << 40), DFOT_ERR_SHAPE, "op_mha_packed: seqs=%d x len=%d x heads=%d is too large", seqs,
               len, heads);
  const float scale2 = 1.4426950408889634f / 8.0f;  // softmax(s / sqrt(64)) in the exp2 domain
  hipLaunchKernelGGL(mha_packed_kernel, dim3((unsigned)blocks), dim3(MHA_THREADS), 0, (hipStream_t)stream, (const bf16*)qkv, (bf16*)o, (long)ld,
                     (long)heads * 64, len, heads, nqb, scale2);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_layernorm(const float* x, const float* gamma, const float* beta, float eps, void* out_bf16, float* out_f32, int64_t rows, int channels,
                      int seq_len, int first, int take, void* stream) {
  DFOT_REQUIRE(x && gamma && beta && (out_bf16 || out_f32) && (const void*)x != out_bf16, DFOT_ERR_ARG, "op_layernorm: null or aliased argument");
  DFOT_REQUIRE(rows > 0 && rows < (1L << 31) && width_ok(channels), DFOT_ERR_SHAPE, "op_layernorm: rows=%ld of channels=%d (512, 768 or 1024)",
               (long)rows, channels);
  DFOT_REQUIRE(seq_len == 0 ? (first == 0 && take == 0) : (first >= 0 && take >= 1 && first + take <= seq_len && rows % take == 0 && x != out_f32),
               DFOT_ERR_SHAPE, "op_layernorm: gather of take=%d rows from first=%d of every seq_len=%d rows into rows=%ld (whole sequences, not in place)",
               take, first, seq_len, (long)rows);
  hipLaunchKernelGGL(layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, (bf16*)out_bf16, out_f32, (long)rows,
                     channels, seq_len, first, take);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_bias_act_bf16(const float* x, int64_t ld, const float* bias, void* out, int64_t rows, int n, int act, void* stream) {
  DFOT_REQUIRE(x && bias && out, DFOT_ERR_ARG, "op_bias_act_bf16: null argument");
  DFOT_REQUIRE(rows > 0 && n > 0 && n % 4 == 0 && ld >= n && ld % 4 == 0 && (act == 0 || act == 1) && rows * (n / 4) < (1L << 40), DFOT_ERR_SHAPE,
               "op_bias_act_bf16: rows=%ld x n=%d (a multiple of 4) with row stride ld=%ld, act=%d (0 GELU-erf, 1 tanh)", (long)rows, n, (long)ld, act);
  const long total4 = rows * (n / 4);
  hipLaunchKernelGGL(bias_act_kernel, dim3(cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream, x, (long)ld, bias, (bf16*)out, total4, n / 4, act);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_titok_tokens(const float* z, const float* embed_w, const float* embed_b, const float* latent_pos, const float* cls, const float* mask_token,
                         const float* pos, const float* gamma, const float* beta, float eps, float* out, int frames, int grid2, int num_latent,
                         int token_size, int channels, int l2norm, void* stream) {
  DFOT_REQUIRE(z && embed_w && embed_b && latent_pos && cls && mask_token && pos && gamma && beta && out, DFOT_ERR_ARG, "op_titok_tokens: null argument");
  DFOT_REQUIRE(frames > 0 && grid2 >= 1 && num_latent >= 1 && token_size >= 1 && token_size <= TOK_MAX_TS && width_ok(channels) &&
                   (long)frames * (1 + grid2 + num_latent) < (1L << 31),
               DFOT_ERR_SHAPE, "op_titok_tokens: frames=%d grid2=%d num_latent=%d token_size=%d (1 .. %d) channels=%d (512, 768 or 1024)", frames, grid2,
               num_latent, token_size, TOK_MAX_TS, channels);
  const long rows = (long)frames * (1 + grid2 + num_latent);
  hipLaunchKernelGGL(titok_tokens_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, z, embed_w, embed_b, latent_pos, cls, mask_token, pos,
                     gamma, beta, eps, out, rows, grid2, num_latent, token_size, channels, l2norm);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_titok_patch_rows(const float* frames, void* rows_bf16, int nframes, int image_size, void* stream) {
  DFOT_REQUIRE(frames && rows_bf16 && (const void*)frames != rows_bf16, DFOT_ERR_ARG, "op_titok_patch_rows: null or aliased argument");
  DFOT_REQUIRE(nframes > 0 && image_size >= 16 && image_size % 16 == 0 && image_size <= 4096 &&
                   (long)nframes * (image_size / 16) * (image_size / 16) < (1L << 31) / 96,
               DFOT_ERR_SHAPE, "op_titok_patch_rows: nframes=%d frames of image_size=%d (a positive multiple of 16, up to 4096; nframes * (image_size / 16)^2 "
               "rows below 2^31 / 96)", nframes, image_size);
  const int g = image_size / 16;
  const long total8 = (long)nframes * g * g * 96;
  hipLaunchKernelGGL(titok_patch_rows_kernel, dim3(cdiv(total8, 256)), dim3(256), 0, (hipStream_t)stream, frames, (bf16*)rows_bf16, total8, image_size, g);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_titok_enc_tokens(const float* patches, int64_t ldp, const float* cls, const float* pos, const float* latent_tokens, const float* latent_pos,
                             const float* gamma, const float* beta, float eps, float* out, int frames, int grid2, int num_latent, int channels,
                             void* stream) {
  DFOT_REQUIRE(patches && cls && pos && latent_tokens && latent_pos && gamma && beta && out && patches != out, DFOT_ERR_ARG,
               "op_titok_enc_tokens: null or aliased argument");
  DFOT_REQUIRE(frames > 0 && grid2 >= 1 && num_latent >= 1 && width_ok(channels) && ldp >= channels && ldp % 4 == 0 &&
                   (long)frames * (1 + grid2 + num_latent) < (1L << 31),
               DFOT_ERR_SHAPE, "op_titok_enc_tokens: frames=%d grid2=%d num_latent=%d channels=%d (512, 768 or 1024), patch row stride ldp=%ld (>= channels, a "
               "multiple of 4)", frames, grid2, num_latent, channels, (long)ldp);
  const long rows = (long)frames * (1 + grid2 + num_latent);
  hipLaunchKernelGGL(titok_enc_tokens_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, patches, (long)ldp, cls, pos, latent_tokens,
                     latent_pos, gamma, beta, eps, out, rows, grid2, num_latent, channels);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_titok_moments(const float* t, const float* w, const float* bias, float* out, int64_t ldo, int frames, int num_latent, int channels,
                          int out_channels, void* stream) {
  DFOT_REQUIRE(t && w && bias && out && t != out, DFOT_ERR_ARG, "op_titok_moments: null or aliased argument");
  DFOT_REQUIRE(frames > 0 && num_latent >= 1 && num_latent <= 128 && width_ok(channels) && out_channels >= 2 && out_channels <= 128 &&
                   out_channels % 2 == 0 && ldo >= out_channels && (long)frames * (out_channels / 2) < (1L << 31),
               DFOT_ERR_SHAPE, "op_titok_moments: frames=%d num_latent=%d (1 .. 128) channels=%d (512, 768 or 1024) out_channels=%d (even, 2 .. 128), row "
               "stride ldo=%ld (>= out_channels)", frames, num_latent, channels, out_channels, (long)ldo);
  const int pairs = out_channels / 2;
  hipLaunchKernelGGL(titok_moments_kernel, dim3((unsigned)((long)frames * pairs)), dim3(256), 0, (hipStream_t)stream, t, w, bias, out, (long)ldo,
                     num_latent, channels, pairs);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // extern "C"
