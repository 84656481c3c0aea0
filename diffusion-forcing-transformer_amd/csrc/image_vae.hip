// ImageVAE pieces (algorithms/vae/image_vae/model.py:18-245, algorithms/vae/common/modules/{attention,updownsample}.py): the per-frame
// Stable-Diffusion-style autoencoder of the DMLab / Minecraft latent recipes.  Its stride-1 convolutions, 1x1 projections, GroupNorm and
// pixel pack are the ops of vae.hip / gemm.hip; this file adds the three layers that had no op.  Activations are channels-last
// [frames][H][W][C]; bf16 GEMM operands, fp32 accumulation and fp32 streams.
//   dfot_op_ivae_attention     AttnBlock (attention.py:39-83): per frame ONE head over the N = H*W positions with all C channels, every
//                              frame in one launch, no score matrix in HBM.  A workgroup owns 32 query rows per wave of one frame and
//                              streams K, then V, through LDS in 64-channel chunks [N][64]:
//                                S^T (keys x q) = K Q^T accumulates over the channel chunks in registers (N/32 MFMA tiles per wave),
//                                softmax over the keys in fp32 with the row max subtracted (lane-local + one exchange with lane^32),
//                                P rounded to bf16, O^T (64 channels x q) = V^T P^T per output-column chunk, scaled by 1 / sum and stored.
//                              The S^T accumulator registers are the B operand of the second product (attention.hip's idiom), the V^T
//                              operand is a transposed LDS read of the chunk image of attention_common.h (AttnCfg<64>).
//                              That form holds all N scores of a row in registers: N = 64 and 256 (64^2 and 128^2 frames).  A multiple
//                              of 256 in [512, 4096] (1024 = a 256^2 frame, 4096 = a 512^2 frame) runs ivae_attn_stream_kernel: keys in
//                              blocks of 128 with a running max and sum, the 4 waves of a workgroup sharing 32 query rows (see there).
//   dfot_op_conv3x3_s2_f32     Downsample (updownsample.py:27-45): F.pad(x, (0, 1, 0, 1)) + Conv2d(k 3, s 2, p 0) as an implicit GEMM:
//                              source pixel (2 y + dy, 2 x + dx), rows / columns past the image are the zero padding (bottom / right only)
//   dfot_op_upconv3x3_f32      Upsample (updownsample.py:10-24): nearest 2x + Conv2d(k 3, s 1, p 1) as ONE implicit GEMM whose gather reads
//                              source pixel ((y + dy - 1) >> 1, (x + dx - 1) >> 1): the 4x-sized intermediate never exists
// Both convolutions are one kernel (conv_kernel<MODE>): 128 x 128 output tile, 4 waves of 64 x 64 (2 x 2 mfma_f32_32x32x16_bf16), K tiles
// of 64 channels of one tap, operands staged global -> registers -> LDS (two stages, XOR-swizzled 16-byte chunks), the next tile's loads
// in flight during the current tile's MFMAs.  K is summed in one fixed order whatever the number of frames.
#include "attention_common.h"
#include "common.h"
#include "dfot_hip.h"

namespace dfot {
namespace {

enum ConvMode { CONV_S2 = 0, CONV_UP = 1 };

constexpr int CT = 128;       // output tile: CT rows (pixels) x CT columns (output channels)
constexpr int CK = 64;        // K tile: 64 channels of one tap
constexpr int CROWB = CK * 2; // bytes of one LDS row

__device__ __forceinline__ int cswz(int row, int c) { return c ^ (row & 7); }

template <int MODE>
__global__ __launch_bounds__(256) void conv_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ y, int M, int hin, int win, int ho, int wo, int cin, int cout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][A tile 16 KB | W tile 16 KB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * CT, n0 = blockIdx.y * CT;
  const int K = 9 * cin;

  // this thread stages chunk `ch` (8 channels) of rows tid/8 + 32 i, i = 0..3, of both tiles
  const int ch = tid & 7;
  int a_y[4], a_x[4];
  long a_base[4];  // element offset of the row's frame; < 0: a row past M
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + (tid >> 3) + 32 * i;
    const int xo = m % wo, yo = (m / wo) % ho;
    const long f = m / (wo * ho);
    a_base[i] = m < M ? f * hin * win * cin : -1;
    a_y[i] = MODE == CONV_S2 ? 2 * yo : yo - 1;
    a_x[i] = MODE == CONV_S2 ? 2 * xo : xo - 1;
  }
  bf16x8 ra[4], rw[4];
  auto load_tile = [&](int kt) {
    const int k0 = kt * CK;
    const int tap = k0 / cin, c0 = k0 - tap * cin + ch * 8;
    const int dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int yy = a_y[i] + dy, xx = a_x[i] + dx;
      bool ok = a_base[i] >= 0;
      if (MODE == CONV_S2) {
        ok = ok && yy < hin && xx < win;
      } else {
        ok = ok && yy >= 0 && xx >= 0 && yy < 2 * hin && xx < 2 * win;
        yy >>= 1;
        xx >>= 1;
      }
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = f2bf(0.f);
      if (ok) v = *reinterpret_cast<const bf16x8*>(x + a_base[i] + ((long)yy * win + xx) * cin + c0);
      ra[i] = v;
      rw[i] = *reinterpret_cast<const bf16x8*>(w + (long)(n0 + (tid >> 3) + 32 * i) * K + k0 + ch * 8);
    }
  };
  auto store_tile = [&](int stage) {
    char* sa = smem + stage * 2 * CT * CROWB;
    char* sw = sa + CT * CROWB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (tid >> 3) + 32 * i;
      *reinterpret_cast<bf16x8*>(sa + row * CROWB + cswz(row, ch) * 16) = ra[i];
      *reinterpret_cast<bf16x8*>(sw + row * CROWB + cswz(row, ch) * 16) = rw[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int nkt = K / CK;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const char* sa = smem + (kt & 1) * 2 * CT * CROWB;
    const char* sw = sa + CT * CROWB;
    if (kt + 1 < nkt) load_tile(kt + 1);
#pragma unroll
    for (int ks = 0; ks < CK / 16; ++ks) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int ar = wm * 64 + i * 32 + lq, br = wn * 64 + i * 32 + lq;
        af[i] = *reinterpret_cast<const bf16x8*>(sa + ar * CROWB + cswz(ar, ks * 2 + lh) * 16);
        bf[i] = *reinterpret_cast<const bf16x8*>(sw + br * CROWB + cswz(br, ks * 2 + lh) * 16);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bf[b], acc[a][b], 0, 0, 0);
    }
    if (kt + 1 < nkt) store_tile((kt + 1) & 1);
    __syncthreads();
  }

  // acc[a][b][r]: row m0 + wm*64 + a*32 + (r&3) + 8*(r>>2) + 4*lh, column n0 + wn*64 + b*32 + lq
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = n0 + wn * 64 + b * 32 + lq;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < M) y[(long)row * cout + col] = acc[a][b][r] + bv;
      }
  }
}

template <int MODE>
int launch_conv(const void* x, const void* w, const float* bias, float* y, int frames, int h_in, int w_in, int cin, int cout, hipStream_t s,
                const char* what) {
  DFOT_REQUIRE(x && w && y && x != (const void*)y, DFOT_ERR_ARG, "%s: null or aliased argument", what);
  DFOT_REQUIRE(frames > 0 && h_in > 0 && w_in > 0 && (MODE == CONV_UP || (h_in % 2 == 0 && w_in % 2 == 0)), DFOT_ERR_SHAPE,
               "%s: %d frames of %dx%d (positive, even for the stride-2 convolution)", what, frames, h_in, w_in);
  DFOT_REQUIRE(cin > 0 && cin % CK == 0 && cout > 0 && cout % CT == 0, DFOT_ERR_SHAPE, "%s: Cin=%d must be a multiple of %d, Cout=%d of %d", what,
               cin, CK, cout, CT);
  const int ho = MODE == CONV_S2 ? h_in / 2 : 2 * h_in, wo = MODE == CONV_S2 ? w_in / 2 : 2 * w_in;
  const long m = (long)frames * ho * wo;
  DFOT_REQUIRE(m < (1L << 31) && (long)frames * h_in * w_in * cin < (1L << 40), DFOT_ERR_SHAPE, "%s: M=%ld rows", what, m);
  constexpr int lds = 2 * 2 * CT * CROWB;
  int rc = ensure_dyn_lds<conv_kernel<MODE>>(lds);
  if (rc) return rc;
  hipLaunchKernelGGL((conv_kernel<MODE>), dim3(cdiv(m, CT), cout / CT), dim3(256), lds, s, (const bf16*)x, (const bf16*)w, bias, y, (int)m, h_in,
                     w_in, ho, wo, cin, cout);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// N: positions per frame; WAVES: waves per workgroup (32 query rows each).  Chunk image: [N][64] bf16 as N / 64 tiles of AttnCfg<64>
// (row r of the chunk at byte r * 128: the tiles are contiguous and the swizzles depend on the low row bits only).
template <int N, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ivae_attn_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                               const bf16* __restrict__ V, bf16* __restrict__ O, int C, float scale2) {
  using Cfg = AttnCfg<64>;
  constexpr int THREADS = WAVES * 64;
  constexpr int QB = WAVES * 32;            // query rows per workgroup
  constexpr int NT = N / 32;                // 32-key MFMA tiles
  constexpr int PER = N * 8 / THREADS;      // 16-byte chunks each thread stages per [N][64] image
  constexpr int IMG = N * Cfg::ROWB;        // bytes of one chunk image
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][IMG]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int frame = blockIdx.x / (N / QB);
  const int q0 = (blockIdx.x % (N / QB)) * QB + wave * 32;
  const long fbase = (long)frame * N * C;
  const int nc = C / 64;

  bf16x8 stg[PER], qn[4];
  auto load_chunk = [&](int i) {            // chunk i < nc: K channels 64 i ..; else V channels 64 (i - nc) ..
    const bf16* src = (i < nc ? K : V) + fbase + (i < nc ? i : i - nc) * 64;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + THREADS * j;
      stg[j] = *reinterpret_cast<const bf16x8*>(src + (long)(e >> 3) * C + (e & 7) * 8);
    }
    if (i < nc) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qn[ks] = *reinterpret_cast<const bf16x8*>(Q + fbase + (long)(q0 + lq) * C + i * 64 + ks * 16 + lh * 8);
    }
  };
  auto store_chunk = [&](int i) {
    char* dst = smem + (i & 1) * IMG;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + THREADS * j;
      const int row = e >> 3, c = e & 7;
      *reinterpret_cast<bf16x8*>(dst + row * Cfg::ROWB + (i < nc ? Cfg::swz_k(row, c) : Cfg::swz_v(row, c)) * 16) = stg[j];
    }
  };

  // ---- S^T = K Q^T, accumulated over the channel chunks ----
  f32x16 sacc[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.f;
  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int i = 0; i < nc; ++i) {
    const char* sk = smem + (i & 1) * IMG;
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
    load_chunk(i + 1);                      // chunk nc (the first V chunk) follows the last K chunk
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      const int row = kt * 32 + lq;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + row * Cfg::ROWB + Cfg::swz_k(row, ks * 2 + lh) * 16);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc[kt], 0, 0, 0);
      }
    }
    store_chunk(i + 1);
    __syncthreads();
  }

  // ---- softmax over the keys of one query column: 16 NT scores in this lane, the other 16 NT in lane ^ 32 ----
  float mx = sacc[0][0];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kt][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float rs = 0.f;
  bf16x8 pf[NT][2];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f((sacc[kt][8 * s + j] - mx) * scale2);
        rs += p;
        pf[kt][s][j] = f2bf(p);             // P.V takes bf16 operands
      }
  const float inv = 1.0f / (rs + __shfl_xor(rs, 32));

  // ---- O^T = V^T P^T, one 64-channel output chunk at a time ----
  bf16* orow = O + fbase + (long)(q0 + lq) * C;
  for (int i = nc; i < 2 * nc; ++i) {
    const char* sv = smem + (i & 1) * IMG;
    if (i + 1 < 2 * nc) load_chunk(i + 1);
    f32x16 oacc[2];
#pragma unroll
    for (int dvt = 0; dvt < 2; ++dvt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dvt][r] = 0.f;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_v<64>(sv + (kt >> 1) * Cfg::TILE, dvt, kt & 1, s, lane), pf[kt][s], oacc[dvt], 0,
                                                              0, 0);
    }
    // lane holds O[q0 + lq][64 (i - nc) + 32 dvt + 8 g + 4 lh + {0..3}] in oacc[dvt][4 g .. 4 g + 3]
#pragma unroll
    for (int dvt = 0; dvt < 2; ++dvt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf16x4 o4;
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = f2bf(oacc[dvt][4 * g4 + j] * inv);
        *reinterpret_cast<bf16x4*>(orow + (i - nc) * 64 + dvt * 32 + 8 * g4 + 4 * lh) = o4;
      }
    if (i + 1 < 2 * nc) store_chunk(i + 1);
    __syncthreads();
  }
}

template <int N, int WAVES>
int launch_ivae_attn(const bf16* q, const bf16* k, const bf16* v, bf16* o, int frames, int c, hipStream_t s) {
  constexpr int lds = 2 * N * AttnCfg<64>::ROWB;
  int rc = ensure_dyn_lds<ivae_attn_kernel<N, WAVES>>(lds);
  if (rc) return rc;
  const float scale2 = 1.4426950408889634f / sqrtf((float)c);  // softmax(s / sqrt(C)) in the exp2 domain
  hipLaunchKernelGGL((ivae_attn_kernel<N, WAVES>), dim3(frames * (N / (WAVES * 32))), dim3(WAVES * 64), lds, s, q, k, v, o, c, scale2);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Streaming form for N >= 512 (a multiple of SKB): the scores of a query row no longer fit the register file, so the keys go by in
// blocks of SKB = 128 with a running row max and sum (online softmax).  CPW = C / 128: 32-channel output blocks per wave.
// The 4 waves of a workgroup share ONE tile of 32 query rows and split each key block two ways:
//   scores   wave w forms S^T (32 keys x 32 q) of keys 32 w .. of the block over all C channels: K chunks [128][64] through LDS
//            (the chunk image of the kernel above), Q fragments from the resident Q image [C / 64][32][64];
//   softmax  per-wave row max -> LDS -> block max of the 4 waves in wave order, m = max(m, block max); p = exp2((s - m) scale2),
//            rounded to bf16 and published in LDS as the B fragments of the second product, the per-wave row sums next to it;
//            l = l alpha + (sum 0 + sum 1 + sum 2 + sum 3), O^T *= alpha, alpha = exp2((m_old - m) scale2): every wave keeps the
//            same (m, l) of its lane's query row;
//   P.V      wave w owns output channels 128 j + 32 w .. + 32, j < CPW (16 CPW accumulator registers): V stages [64 keys][128
//            channels] as two AttnCfg<64> tiles; the wave reads the V^T fragments of tile w >> 1, column block w & 1, and multiplies
//            with all four P slices.
// One stage is 16 KB; the global -> register -> LDS pipeline of the kernel above runs through the K chunks and V stages of all key
// blocks in one sequence (two stages in LDS).  Everything is summed in one fixed order that depends on (N, C) only.
constexpr int SKB = 128;                   // keys per block
constexpr int SQB = 32;                    // query rows per workgroup
constexpr int SSTAGE = 16384;              // bytes of one K chunk [128][64] or V stage 2 x [64][64]

template <int CPW>
__global__ __launch_bounds__(256) void ivae_attn_stream_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                               const bf16* __restrict__ V, bf16* __restrict__ O, int N, float scale2) {
  using Cfg = AttnCfg<64>;
  constexpr int C = 128 * CPW;
  constexpr int NKC = C / 64;              // K chunks of a key block
  constexpr int NVS = 2 * CPW;             // V stages of a key block: (channel group j, key half h)
  constexpr int QIMG = SQB * Cfg::ROWB;    // bytes of one 64-channel chunk of the Q image
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][SSTAGE] | Q image NKC * QIMG | P 4 x 2 x 64 x 16 | max 4 x 32 | sum 4 x 32
  char* const sq = smem + 2 * SSTAGE;
  char* const sp = sq + NKC * QIMG;
  float* const smax = reinterpret_cast<float*>(sp + 4 * 2 * 64 * 16);
  float* const ssum = smax + 4 * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int qblocks = N / SQB;
  const int frame = blockIdx.x / qblocks;
  const int q0 = (blockIdx.x % qblocks) * SQB;
  const long fbase = (long)frame * N * C;
  const int nblk = N / SKB;

  bf16x8 stg[4];
  auto load_k = [&](int kb0, int i) {      // K rows kb0 .. kb0 + 128, channels 64 i .. 64 i + 64
    const bf16* src = K + fbase + (long)kb0 * C + i * 64;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + 256 * j;
      stg[j] = *reinterpret_cast<const bf16x8*>(src + (long)(e >> 3) * C + (e & 7) * 8);
    }
  };
  auto store_k = [&](int buf) {
    char* dst = smem + buf * SSTAGE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + 256 * j;
      const int row = e >> 3, c = e & 7;
      *reinterpret_cast<bf16x8*>(dst + row * Cfg::ROWB + Cfg::swz_k(row, c) * 16) = stg[j];
    }
  };
  auto load_v = [&](int kb0, int t) {      // stage t = 2 j + h: V rows kb0 + 64 h .. + 64, channels 128 j .. 128 j + 128
    const bf16* src = V + fbase + (long)(kb0 + 64 * (t & 1)) * C + (t >> 1) * 128;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + 256 * j;
      stg[j] = *reinterpret_cast<const bf16x8*>(src + (long)(e >> 4) * C + (e & 15) * 8);
    }
  };
  auto store_v = [&](int buf) {
    char* dst = smem + buf * SSTAGE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + 256 * j;
      const int row = e >> 4, c = e & 7;
      *reinterpret_cast<bf16x8*>(dst + ((e >> 3) & 1) * Cfg::TILE + row * Cfg::ROWB + Cfg::swz_v(row, c) * 16) = stg[j];
    }
  };

  // ---- the Q image: chunk i holds rows q0 .. q0 + 32, channels 64 i .. 64 i + 64, in the K chunk's row layout ----
  {
    const int row = tid >> 3, c = tid & 7;
#pragma unroll
    for (int i = 0; i < NKC; ++i)
      *reinterpret_cast<bf16x8*>(sq + i * QIMG + row * Cfg::ROWB + Cfg::swz_k(row, c) * 16) =
          *reinterpret_cast<const bf16x8*>(Q + fbase + (long)(q0 + row) * C + i * 64 + c * 8);
  }
  load_k(0, 0);
  store_k(0);
  __syncthreads();

  f32x16 oacc[CPW];
#pragma unroll
  for (int j = 0; j < CPW; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[j][r] = 0.f;
  float m = -INFINITY, l = 0.f;            // of query row q0 + lq, the same in the 8 lanes (4 waves x 2 halves) that hold it

  for (int blk = 0; blk < nblk; ++blk) {
    const int kb0 = blk * SKB;
    // ---- S^T = K Q^T for this wave's 32 keys ----
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
    for (int i = 0; i < NKC; ++i) {
      const char* sk = smem + (i & 1) * SSTAGE;
      if (i + 1 < NKC) load_k(kb0, i + 1); else load_v(kb0, 0);
      const int row = wave * 32 + lq;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + row * Cfg::ROWB + Cfg::swz_k(row, ks * 2 + lh) * 16);
        const bf16x8 qf = *reinterpret_cast<const bf16x8*>(sq + i * QIMG + lq * Cfg::ROWB + Cfg::swz_k(lq, ks * 2 + lh) * 16);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf, sacc, 0, 0, 0);
      }
      if (i + 1 < NKC) store_k((i + 1) & 1); else store_v(0);   // NKC is even: V stage 0 goes to buffer 0
      __syncthreads();
    }

    // ---- online softmax: 16 of this wave's 32 scores of query lq are in this lane, the other 16 in lane ^ 32 ----
    float mx = sacc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (lh == 0) smax[wave * 32 + lq] = mx;
    __syncthreads();
    float mnew = m;
#pragma unroll
    for (int w = 0; w < 4; ++w) mnew = fmaxf(mnew, smax[w * 32 + lq]);
    const float alpha = __builtin_amdgcn_exp2f((m - mnew) * scale2);   // 0 in the first block (m = -inf)
    m = mnew;
    float rs = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f((sacc[8 * s + j] - mnew) * scale2);
        rs += p;
        pf[j] = f2bf(p);                   // P.V takes bf16 operands
      }
      *reinterpret_cast<bf16x8*>(sp + ((wave * 2 + s) * 64 + lane) * 16) = pf;
    }
    rs += __shfl_xor(rs, 32);
    if (lh == 0) ssum[wave * 32 + lq] = rs;
    __syncthreads();
    l = l * alpha + (((ssum[lq] + ssum[32 + lq]) + ssum[64 + lq]) + ssum[96 + lq]);
#pragma unroll
    for (int j = 0; j < CPW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[j][r] *= alpha;
    bf16x8 pf[4][2];                       // the whole P block as B fragments: key tile kt (the slice of wave kt), 16-key step s
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) pf[kt][s] = *reinterpret_cast<const bf16x8*>(sp + ((kt * 2 + s) * 64 + lane) * 16);

    // ---- O^T += V^T P^T for this wave's channels ----
#pragma unroll
    for (int t = 0; t < NVS; ++t) {
      const char* sv = smem + (t & 1) * SSTAGE + (wave >> 1) * Cfg::TILE;
      const bool more = t + 1 < NVS || blk + 1 < nblk;
      if (t + 1 < NVS) load_v(kb0, t + 1); else if (more) load_k(kb0 + SKB, 0);
#pragma unroll
      for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          oacc[t >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_v<64>(sv, wave & 1, kt2, s, lane), pf[2 * (t & 1) + kt2][s],
                                                                 oacc[t >> 1], 0, 0, 0);
      if (t + 1 < NVS) store_v((t + 1) & 1); else if (more) store_k(0);   // NVS is even: the next block's K chunk 0 goes to buffer 0
      __syncthreads();
    }
  }

  // lane holds O[q0 + lq][128 j + 32 wave + 8 g + 4 lh + {0..3}] in oacc[j][4 g .. 4 g + 3]
  const float inv = 1.0f / l;
  bf16* orow = O + fbase + (long)(q0 + lq) * C + 32 * wave + 4 * lh;
#pragma unroll
  for (int j = 0; j < CPW; ++j)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 o4;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) o4[jj] = f2bf(oacc[j][4 * g4 + jj] * inv);
      *reinterpret_cast<bf16x4*>(orow + 128 * j + 8 * g4) = o4;
    }
}

template <int CPW>
int launch_ivae_attn_stream(const bf16* q, const bf16* k, const bf16* v, bf16* o, int frames, int n, hipStream_t s) {
  constexpr int lds = 2 * SSTAGE + 2 * CPW * SQB * AttnCfg<64>::ROWB + 4 * 2 * 64 * 16 + 2 * 4 * 32 * (int)sizeof(float);
  static_assert(lds <= 160 * 1024, "the streaming attention kernel's LDS exceeds one CU");
  int rc = ensure_dyn_lds<ivae_attn_stream_kernel<CPW>>(lds);
  if (rc) return rc;
  const float scale2 = 1.4426950408889634f / sqrtf(128.f * CPW);  // softmax(s / sqrt(C)) in the exp2 domain
  hipLaunchKernelGGL((ivae_attn_stream_kernel<CPW>), dim3(frames * (n / SQB)), dim3(256), lds, s, q, k, v, o, n, scale2);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace
}  // namespace dfot

extern "C" {
using namespace dfot;

int dfot_op_ivae_attention(const void* q, const void* k, const void* v, void* o, int frames, int n, int c, void* stream) {
  DFOT_REQUIRE(q && k && v && o && o != q && o != k && o != v, DFOT_ERR_ARG, "op_ivae_attention: null or aliased argument");
  const bool stream_n = n >= 512 && n <= 4096 && n % 256 == 0;
  DFOT_REQUIRE(frames > 0 && (n == 64 || n == 256 || stream_n) && c >= 128 && c % 128 == 0 && c <= 1024 && (long)frames * (n / 64) < (1L << 30),
               DFOT_ERR_SHAPE,
               "op_ivae_attention: %d frames of N=%d positions with C=%d channels (N in {64, 256} or a multiple of 256 in [512, 4096], C a "
               "multiple of 128 up to 1024)", frames, n, c);
  hipStream_t s = (hipStream_t)stream;
  if (n == 64) return launch_ivae_attn<64, 2>((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, frames, c, s);
  if (n == 256) return launch_ivae_attn<256, 4>((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, frames, c, s);
  switch (c / 128) {
#define DFOT_IVAE_STREAM(CPW) \
  case CPW: return launch_ivae_attn_stream<CPW>((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, frames, n, s)
    DFOT_IVAE_STREAM(1);
    DFOT_IVAE_STREAM(2);
    DFOT_IVAE_STREAM(3);
    DFOT_IVAE_STREAM(4);
    DFOT_IVAE_STREAM(5);
    DFOT_IVAE_STREAM(6);
    DFOT_IVAE_STREAM(7);
    DFOT_IVAE_STREAM(8);
#undef DFOT_IVAE_STREAM
  }
  DFOT_REQUIRE(false, DFOT_ERR_SHAPE, "op_ivae_attention: C=%d", c);
  return DFOT_ERR_SHAPE;
}

int dfot_op_conv3x3_s2_f32(const void* x, const void* w, const float* bias, float* y, int frames, int h_in, int w_in, int cin, int cout,
                           void* stream) {
  return launch_conv<CONV_S2>(x, w, bias, y, frames, h_in, w_in, cin, cout, (hipStream_t)stream, "op_conv3x3_s2_f32");
}

int dfot_op_upconv3x3_f32(const void* x, const void* w, const float* bias, float* y, int frames, int h_in, int w_in, int cin, int cout,
                          void* stream) {
  return launch_conv<CONV_UP>(x, w, bias, y, frames, h_in, w_in, cin, cout, (hipStream_t)stream, "op_upconv3x3_f32");
}

}  // extern "C"
