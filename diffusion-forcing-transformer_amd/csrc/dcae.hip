// DC-AE pieces (algorithms/vae/dc_ae/autoencoder_dc_model.py:45-466): the deep-compression autoencoder whose 32-channel 8x8 latents the
// dmlab / Minecraft recipes run in.  Its 3x3 convolutions and 1x1 projections are the ops of vae.hip / gemm.hip; this file adds the layers
// that had no op.  Activations are channels-last [frames][H][W][C]; bf16 GEMM operands, fp32 streams and fp32 arithmetic throughout.
//   dfot_op_dcae_linear_attention   ReLU linear attention (SanaMultiscaleLinearAttention.apply_linear_attention, :86-95).  One workgroup
//                                   of 4 waves per (frame, head).  2 * 33 * 32 * N FLOP per head and direction is nothing: the kernel is
//                                   bound by the latency of reading N x 96 bf16 twice, so the work is laid out for few dependent steps,
//                                   not for the matrix cores.  Pass 1: K and V go through LDS in chunks of 64 positions as fp32 (ReLU
//                                   applied to K); thread (j, dg) owns S[j][4 dg .. 4 dg + 3] and the key sum S[j][32] and adds the 64
//                                   positions in ascending order.  Pass 2: thread (position, 8-channel group) reads its q row from global
//                                   memory, contracts it with the 32 x 33 state in LDS and divides.  The summation order depends on N only.
//   dfot_op_dcae_dw_glu             GLUMBConv's depthwise 3x3 + bias + x * silu(gate).  A workgroup owns a slab of 256 channels of both
//                                   halves (their 9 x 512 weights in LDS, 18 KB) and 16 pixels; a thread owns 8 channels (16-byte loads of
//                                   both halves per tap, one 16-byte store) of two pixels, 8 apart.
//   dfot_op_dcae_down_shortcut      pixel_unshuffle + channel-group mean   (DCDownBlock2d, the encoder's output shortcut with factor 1)
//   dfot_op_dcae_up_shortcut        pixel_shuffle + channel repeat         (DCUpBlock2d, the decoder's input shortcut with factor 1)
//   dfot_op_dcae_rmsnorm            channel RMSNorm with weight and bias, (+ residual) (+ ReLU), fp32 and / or bf16 out; one wave per row
//   dfot_op_dcae_act_bf16           ReLU / SiLU + bf16 cast (a ResBlock's activation in front of conv2)
// Rows a work item does not own: every kernel indexes by (frame, position) below frames * N; the rows that pad a GEMM operand to whole tiles
// are never read or written here.
#include "common.h"
#include "dfot_hip.h"

namespace dfot {
namespace {

constexpr int LA_CHUNK = 64;   // positions per LDS chunk
constexpr int LA_D = 32;       // head dimension
constexpr int LA_SLD = 36;     // row stride of the state: 33 columns, padded to keep float4 rows aligned

__global__ __launch_bounds__(256) void dcae_linattn_kernel(const bf16* __restrict__ qkv, long ld, bf16* __restrict__ o, long ldo, int n, int heads) {
  __shared__ __attribute__((aligned(16))) float sk[LA_CHUNK][LA_D];
  __shared__ __attribute__((aligned(16))) float sv[LA_CHUNK][LA_D];
  __shared__ __attribute__((aligned(16))) float ss[LA_D][LA_SLD];
  const int tid = threadIdx.x;
  const int frame = blockIdx.x / heads, head = blockIdx.x - frame * heads;
  const bf16* base = qkv + (long)frame * n * ld + head * 3 * LA_D;   // row n0 of this frame, column 96 head: q | k | v

  // ---- pass 1: S[j][d] = sum_n relu(k[n][j]) * [v[n] ; 1][d] ----
  const int j = tid >> 3, dg = tid & 7;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, ks = 0.f;
  for (int n0 = 0; n0 < n; n0 += LA_CHUNK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // 64 rows x (4 k + 4 v) 16-byte pieces
      const int e = tid + 256 * i;
      const int row = e >> 3, c = e & 7;
      const bf16x8 v8 = *reinterpret_cast<const bf16x8*>(base + (long)(n0 + row) * ld + LA_D + c * 8);
      float* dst = c < 4 ? &sk[row][c * 8] : &sv[row][(c - 4) * 8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float f = bf2f(v8[t]);
        dst[t] = c < 4 ? fmaxf(f, 0.f) : f;
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < LA_CHUNK; ++r) {
      const float kk = sk[r][j];
      const f32x4 vv = *reinterpret_cast<const f32x4*>(&sv[r][dg * 4]);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = fmaf(kk, vv[t], acc[t]);
      ks += kk;
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) ss[j][dg * 4 + t] = acc[t];
  if (dg == 0) ss[j][LA_D] = ks;
  __syncthreads();

  // ---- pass 2: o[n][d] = (relu(q[n]) . S[:, d]) / (relu(q[n]) . S[:, 32] + 1e-15) ----
  const int p = tid >> 2, og = tid & 3;
  for (int n0 = 0; n0 < n; n0 += LA_CHUNK) {
    const bf16* qrow = base + (long)(n0 + p) * ld;
    float out[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, den = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bf16x8 q8 = *reinterpret_cast<const bf16x8*>(qrow + c * 8);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float qv = fmaxf(bf2f(q8[t]), 0.f);
        const float* srow = ss[c * 8 + t];
        den = fmaf(qv, srow[LA_D], den);
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = fmaf(qv, srow[og * 8 + i], out[i]);
      }
    }
    den += 1e-15f;
    bf16x8 o8;
#pragma unroll
    for (int i = 0; i < 8; ++i) o8[i] = f2bf(out[i] / den);
    *reinterpret_cast<bf16x8*>(o + ((long)frame * n + n0 + p) * ldo + head * LA_D + og * 8) = o8;
  }
}

constexpr int DW_SLAB = 256;   // channels of each half per workgroup
constexpr int DW_PIX = 16;     // pixels per workgroup: two per thread (the launch is latency-bound at 8 x 8 maps, so the grid is kept wide)

__global__ __launch_bounds__(256) void dcae_dw_glu_kernel(const bf16* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                          bf16* __restrict__ out, long pixels, int h, int w, int hc) {
  __shared__ __attribute__((aligned(16))) float sw[9][2][DW_SLAB];
  const int tid = threadIdx.x;
  const int slab = blockIdx.y;
  const long p0 = (long)blockIdx.x * DW_PIX;
  const long c2 = 2L * hc;
  for (int e = tid; e < 9 * 2 * DW_SLAB / 4; e += 256) {   // 16-byte pieces
    const int tap = e / (2 * DW_SLAB / 4), half = (e / (DW_SLAB / 4)) & 1, c = (e % (DW_SLAB / 4)) * 4;
    *reinterpret_cast<f32x4*>(&sw[tap][half][c]) = *reinterpret_cast<const f32x4*>(wt + tap * c2 + (long)half * hc + slab * DW_SLAB + c);
  }
  __syncthreads();
  const int cg = tid & 31, pl = tid >> 5;
  const int c0 = slab * DW_SLAB + cg * 8;
  float b0[8], b1[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    b0[k] = bias[c0 + k];
    b1[k] = bias[hc + c0 + k];
  }
  for (int i = 0; i < DW_PIX; i += 8) {
    const long pix = p0 + i + pl;
    if (pix >= pixels) break;
    const int xx = (int)(pix % w), yy = (int)((pix / w) % h);
    const long f = pix / ((long)w * h);
    float a0[8], a1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      a0[k] = b0[k];
      a1[k] = b1[k];
    }
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int sy = yy + dy - 1;
      if (sy < 0 || sy >= h) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int sx = xx + dx - 1;
        if (sx < 0 || sx >= w) continue;
        const bf16* src = x + ((f * h + sy) * w + sx) * c2 + c0;
        const bf16x8 u = *reinterpret_cast<const bf16x8*>(src);
        const bf16x8 g = *reinterpret_cast<const bf16x8*>(src + hc);
        const float* w0 = &sw[dy * 3 + dx][0][cg * 8];
        const float* w1 = &sw[dy * 3 + dx][1][cg * 8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          a0[k] = fmaf(bf2f(u[k]), w0[k], a0[k]);
          a1[k] = fmaf(bf2f(g[k]), w1[k], a1[k]);
        }
      }
    }
    bf16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = f2bf(a0[k] * silu_f(a1[k]));
    *reinterpret_cast<bf16x8*>(out + pix * hc + c0) = r;
  }
}

// thread: 4 consecutive output channels of one output pixel
__global__ __launch_bounds__(256) void dcae_down_kernel(const float* __restrict__ conv, long ldc, const float* __restrict__ src, float* __restrict__ out,
                                                        long total, int h, int w, int cin, int cout, int f, int gs) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int q = cout / 4, f2 = f * f;
  const int c4 = (int)(idx % q);
  const long pix = idx / q;
  const int wo = w / f, ho = h / f;
  const int X = (int)(pix % wo), Y = (int)((pix / wo) % ho);
  const long fr = pix / ((long)wo * ho);
  const long row0 = (fr * h + (long)f * Y) * w + (long)f * X;   // source pixel (f Y, f X)
  f32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = c4 * 4 + i;
    const int sub = co % f2;
    float v = conv[(row0 + (long)(sub / f) * w + sub % f) * ldc + co / f2];
    if (src) {
      float s = 0.f;
      for (int k = 0; k < gs; ++k) {
        const long e = (long)co * gs + k;
        const int sb = (int)(e % f2);
        s += src[(row0 + (long)(sb / f) * w + sb % f) * cin + e / f2];
      }
      v += s / (float)gs;
    }
    r[i] = v;
  }
  *reinterpret_cast<f32x4*>(out + pix * cout + c4 * 4) = r;
}

// thread: one output channel of the f x f output pixels of one input pixel
__global__ __launch_bounds__(256) void dcae_up_kernel(const float* __restrict__ conv, long ldc, const float* __restrict__ src, long lds,
                                                      float* __restrict__ out, long total, int h, int w, int cout, int f, int rep) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % cout), f2 = f * f;
  const long pix = idx / cout;
  const int x = (int)(pix % w), y = (int)((pix / w) % h);
  const long fr = pix / ((long)w * h);
  for (int k = 0; k < f2; ++k) {
    const int e = c * f2 + k;
    float v = conv[pix * ldc + e];
    if (src) v += src[pix * lds + e / rep];
    out[((fr * f * h + (long)f * y + k / f) * ((long)f * w) + (long)f * x + k % f) * cout + c] = v;
  }
}

constexpr int RN_MAX4 = 8;   // float4 pieces per lane: channels <= 64 * 4 * 8

__global__ __launch_bounds__(256) void dcae_rmsnorm_kernel(const float* x, const float* __restrict__ wgt, const float* __restrict__ bias, float eps,
                                                           const float* resid, float* out_f32, bf16* out_bf16, int relu, long rows, int channels) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int c4 = channels / 4;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + row * channels);
  f32x4 v[RN_MAX4];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < RN_MAX4; ++i) {
    const int idx = lane + 64 * i;
    if (idx < c4) {
      v[i] = xr[idx];
      ss += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
  const float rs = 1.0f / sqrtf(ss / (float)channels + eps);
#pragma unroll
  for (int i = 0; i < RN_MAX4; ++i) {
    const int idx = lane + 64 * i;
    if (idx < c4) {
      const f32x4 g = reinterpret_cast<const f32x4*>(wgt)[idx], b = reinterpret_cast<const f32x4*>(bias)[idx];
      f32x4 y;
#pragma unroll
      for (int t = 0; t < 4; ++t) y[t] = v[i][t] * rs * g[t] + b[t];
      if (resid) {
        const f32x4 r = reinterpret_cast<const f32x4*>(resid + row * channels)[idx];
#pragma unroll
        for (int t = 0; t < 4; ++t) y[t] += r[t];
      }
      if (relu) {
#pragma unroll
        for (int t = 0; t < 4; ++t) y[t] = fmaxf(y[t], 0.f);
      }
      if (out_f32) reinterpret_cast<f32x4*>(out_f32 + row * channels)[idx] = y;
      if (out_bf16) {
        bf16x4 o4;
#pragma unroll
        for (int t = 0; t < 4; ++t) o4[t] = f2bf(y[t]);
        reinterpret_cast<bf16x4*>(out_bf16 + row * channels)[idx] = o4;
      }
    }
  }
}

__global__ __launch_bounds__(256) void dcae_act_kernel(const f32x4* __restrict__ x, bf16x4* __restrict__ out, long n4, int act) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 v = x[i];
    bf16x4 o4;
#pragma unroll
    for (int t = 0; t < 4; ++t) o4[t] = f2bf(act == 1 ? fmaxf(v[t], 0.f) : act == 2 ? silu_f(v[t]) : v[t]);
    out[i] = o4;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace dfot

extern "C" {
using namespace dfot;

int dfot_op_dcae_linear_attention(const void* qkv, int64_t ld, void* o, int64_t ldo, int frames, int n, int heads, void* stream) {
  DFOT_REQUIRE(qkv && o && qkv != o && aligned16(qkv) && aligned16(o), DFOT_ERR_ARG, "op_dcae_linear_attention: null, aliased or unaligned argument");
  DFOT_REQUIRE(frames > 0 && n >= LA_CHUNK && n <= 4096 && n % LA_CHUNK == 0 && heads >= 1 && heads <= 64 && ld >= 96L * heads && ld % 8 == 0 &&
                   ldo >= 32L * heads && ldo % 8 == 0 && (long)frames * heads < (1L << 31),
               DFOT_ERR_SHAPE,
               "op_dcae_linear_attention: %d frames of N=%d positions, %d heads, ld=%ld, ldo=%ld (N a multiple of 64 in [64, 4096], heads in "
               "[1, 64], ld >= 96 heads, ldo >= 32 heads, both multiples of 8)", frames, n, heads, (long)ld, (long)ldo);
  hipLaunchKernelGGL(dcae_linattn_kernel, dim3(frames * heads), dim3(256), 0, (hipStream_t)stream, (const bf16*)qkv, (long)ld, (bf16*)o, (long)ldo, n,
                     heads);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_dcae_dw_glu(const void* x, const float* w_taps, const float* bias, void* out, int frames, int h, int w, int hc, void* stream) {
  DFOT_REQUIRE(x && w_taps && bias && out && x != out && aligned16(x) && aligned16(out) && aligned16(w_taps), DFOT_ERR_ARG,
               "op_dcae_dw_glu: null, aliased or unaligned argument");
  DFOT_REQUIRE(frames > 0 && h > 0 && w > 0 && hc > 0 && hc % DW_SLAB == 0 && hc <= 65535 * DW_SLAB && (long)frames * h * w < (1L << 31) * DW_PIX,
               DFOT_ERR_SHAPE, "op_dcae_dw_glu: %d frames of %dx%d with %d gated channels (a positive multiple of %d)", frames, h, w, hc, DW_SLAB);
  const long pixels = (long)frames * h * w;
  hipLaunchKernelGGL(dcae_dw_glu_kernel, dim3(cdiv(pixels, DW_PIX), hc / DW_SLAB), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, w_taps, bias,
                     (bf16*)out, pixels, h, w, hc);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_dcae_down_shortcut(const float* conv, int64_t ldc, const float* src, float* out, int frames, int h, int w, int cin, int cout, int factor,
                               void* stream) {
  DFOT_REQUIRE(conv && out && conv != out && src != out && aligned16(out), DFOT_ERR_ARG, "op_dcae_down_shortcut: null, aliased or unaligned argument");
  const int f2 = factor * factor;
  DFOT_REQUIRE(frames > 0 && h > 0 && w > 0 && (factor == 1 || factor == 2) && h % factor == 0 && w % factor == 0 && cout > 0 && cout % 4 == 0 &&
                   cout % f2 == 0 && ldc >= cout / f2 && (!src || (cin > 0 && ((long)f2 * cin) % cout == 0)),
               DFOT_ERR_SHAPE, "op_dcae_down_shortcut: %d frames of %dx%d, Cin=%d, Cout=%d, ldc=%ld, factor %d", frames, h, w, cin, cout, (long)ldc,
               factor);
  const long total = (long)frames * (h / factor) * (w / factor) * (cout / 4);
  DFOT_REQUIRE(total < (1L << 31) * 256, DFOT_ERR_SHAPE, "op_dcae_down_shortcut: %ld work items", total);
  hipLaunchKernelGGL(dcae_down_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, conv, (long)ldc, src, out, total, h, w, cin, cout,
                     factor, src ? f2 * cin / cout : 1);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_dcae_up_shortcut(const float* conv, int64_t ldc, const float* src, int64_t lds, float* out, int frames, int h, int w, int cin, int cout,
                             int factor, void* stream) {
  DFOT_REQUIRE(conv && out && conv != out && src != out, DFOT_ERR_ARG, "op_dcae_up_shortcut: null or aliased argument");
  const int f2 = factor * factor;
  DFOT_REQUIRE(frames > 0 && h > 0 && w > 0 && (factor == 1 || factor == 2) && cout > 0 && ldc >= (long)f2 * cout &&
                   (!src || (cin > 0 && lds >= cin && (f2 * cout) % cin == 0)),
               DFOT_ERR_SHAPE, "op_dcae_up_shortcut: %d frames of %dx%d, Cin=%d, Cout=%d, ldc=%ld, lds=%ld, factor %d", frames, h, w, cin, cout,
               (long)ldc, (long)lds, factor);
  const long total = (long)frames * h * w * cout;
  DFOT_REQUIRE(total < (1L << 31) * 256, DFOT_ERR_SHAPE, "op_dcae_up_shortcut: %ld work items", total);
  hipLaunchKernelGGL(dcae_up_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, conv, (long)ldc, src, (long)lds, out, total, h, w, cout,
                     factor, src ? f2 * cout / cin : 1);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_dcae_rmsnorm(const float* x, const float* weight, const float* bias, float eps, const float* resid, float* out_f32, void* out_bf16,
                         int relu, int64_t rows, int channels, void* stream) {
  DFOT_REQUIRE(x && weight && bias && (out_f32 || out_bf16) && aligned16(x) && aligned16(weight) && aligned16(bias) && aligned16(resid) &&
                   aligned16(out_f32) && aligned16(out_bf16) && (const void*)x != out_bf16,
               DFOT_ERR_ARG, "op_dcae_rmsnorm: null, aliased or unaligned argument");
  DFOT_REQUIRE(rows > 0 && rows < (1L << 32) && channels > 0 && channels % 4 == 0 && channels <= 64 * 4 * RN_MAX4, DFOT_ERR_SHAPE,
               "op_dcae_rmsnorm: %ld rows of %d channels (a multiple of 4 up to %d)", (long)rows, channels, 64 * 4 * RN_MAX4);
  hipLaunchKernelGGL(dcae_rmsnorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, weight, bias, eps, resid, out_f32, (bf16*)out_bf16,
                     relu, (long)rows, channels);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int dfot_op_dcae_act_bf16(const float* x, void* out, int64_t n, int act, void* stream) {
  DFOT_REQUIRE(x && out && (const void*)x != out && aligned16(x) && (reinterpret_cast<uintptr_t>(out) & 7) == 0, DFOT_ERR_ARG,
               "op_dcae_act_bf16: null, aliased or unaligned argument");
  DFOT_REQUIRE(n > 0 && n % 4 == 0 && act >= 0 && act <= 2, DFOT_ERR_SHAPE, "op_dcae_act_bf16: n=%ld (a positive multiple of 4), act=%d in {0, 1, 2}",
               (long)n, act);
  const long n4 = n / 4;
  hipLaunchKernelGGL(dcae_act_kernel, dim3((unsigned)(n4 / 256 < 8192 ? (n4 + 255) / 256 : 8192)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)x,
                     (bf16x4*)out, n4, act);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // extern "C"
