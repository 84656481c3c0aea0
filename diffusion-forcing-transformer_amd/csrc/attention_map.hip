// Attention maps of the DiT3D family (the read-out of the reference's attn_hook): which frame attends to which.  The forward kernels
// never form the score matrix, so these kernels recompute the softmax from the q and k the forward's attention kernel read -- bf16, after
// QK-norm / RoPE, in the forward's layout and pre-scaling -- and write fp32 probabilities.  They read q and k only and are launched only
// when a capture is on; the forward kernels are untouched.
//   full map   A[b][head][i][j] = softmax_j(q_i . k_j)
//   frame map  F[b][head][tq][tk] = (1/P) sum_{i in frame tq} sum_{j in frame tk} A[b][head][i][j]     (P patches per frame; rows sum to 1)
// Every reduction is fixed-order and atomic-free (partials + a finalize launch, as gn_finalize): two calls give the same bits.
//
// 1. attn_map_kernel (variant "full"): q, k [B][heads][N][dstride], N = T * P, q in the exp2 domain (launch_attention_padded's layout).
//    One workgroup = 4 waves = 128 query rows; a wave owns 32 query rows and runs v_mfma_f32_32x32x16_bf16 with Q as the A operand
//    (registers) and a 64-key K tile as the B operand (LDS image and swizzle of attention_common.h), so a lane holds one KEY column and
//    16 query rows: stores of a probability row are 128 contiguous bytes per half wave.  Two passes over the keys:
//      pass 1: running (max, sum) per (lane, query row) over the lane's key columns, merged across the 32 lanes of a row at the end;
//      pass 2: p = exp2(s - max) / sum, then one of two epilogues: FULL stores p to A (the only N x N buffer); FRAME adds p into one
//              per-lane sum per key frame (P % 64 == 0: a key tile lies in one frame, a wave's 32 rows lie in one frame), reduces it
//              over the wave and writes part[b][head][N/32][T]; map_finalize_kernel sums the P/32 row groups of a frame in order.
// 2. attn_temporal_map_kernel (variant "factorized_attention", temporal blocks): the T x T softmax of every (video, head, patch) as
//    attention_temporal.hip computes it (VALU, q / k rows staged in LDS), summed over 64 patches per workgroup in patch order;
//    map_finalize_kernel sums the P/64 workgroups.
// 3. matrix_attn_map_kernel (variant "factorized_matrix_attention"): the score phase of the forward kernel (attention_matrix_scores.h)
//    and its softmax, stored untransposed: [B][col_heads][row_heads][L][L].  Every frame is one token: the full map is the frame map.
#include <algorithm>

#include "attention_common.h"
#include "attention_matrix_scores.h"
#include "kernels.h"

namespace dfot {
namespace {

// merge of two (max, sum) pairs; two rounded products and a rounded (commutative) sum instead of a contracted fma, so that both
// lanes of an exchange compute the same bits
__device__ __forceinline__ void merge_ml(float& m, float& l, float mo, float lo) {
  const float mn = fmaxf(m, mo);
  l = __fadd_rn(__fmul_rn(l, __builtin_amdgcn_exp2f(m - mn)), __fmul_rn(lo, __builtin_amdgcn_exp2f(mo - mn)));
  m = mn;
}

// D: row stride of q / k (64 or 128); DQK: columns multiplied (a multiple of 16 covering d; the pad columns hold zeros)
template <int D, int DQK, bool FULL>
__global__ __launch_bounds__(256) void attn_map_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K, float* __restrict__ out, int N,
                                                       int P, int T) {
  using C = AttnCfg<D>;
  __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int bh = blockIdx.y;
  const long base = (long)bh * N * D;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const bf16* Kb = K + base;

  // Q fragments (A operand): lane holds Q[q0 + lq][16 ks + 8 lh + j]
  bf16x8 qf[DQK / 16];
#pragma unroll
  for (int ks = 0; ks < DQK / 16; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(Q + base + (long)(q0 + lq) * D + ks * 16 + lh * 8);

  bf16x8 rk[C::PER_THREAD];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int i = 0; i < C::PER_THREAD; ++i) {
      const int e = tid + 256 * i;
      const int row = e / C::CH, c = e % C::CH;
      rk[i] = *reinterpret_cast<const bf16x8*>(Kb + (long)(t * C::KV + row) * D + c * 8);
    }
  };
  auto store_tile = [&](int stage) {
    char* sk = smem + stage * C::TILE;
#pragma unroll
    for (int i = 0; i < C::PER_THREAD; ++i) {
      const int e = tid + 256 * i;
      const int row = e / C::CH, c = e % C::CH;
      *reinterpret_cast<bf16x8*>(sk + row * C::ROWB + C::swz_k(row, c) * 16) = rk[i];
    }
  };
  // S (32 queries x 64 keys) of the tile in `sk`: register r of sacc[kt2] = (query (r & 3) + 8 (r >> 2) + 4 lh, key kt2 * 32 + lq)
  auto scores = [&](const char* sk, f32x16 (&sacc)[2]) {
#pragma unroll
    for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[kt2][r] = 0.f;
      const int row = kt2 * 32 + lq;
#pragma unroll
      for (int ks = 0; ks < DQK / 16; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + row * C::ROWB + C::swz_k(row, ks * 2 + lh) * 16);
        sacc[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kf, sacc[kt2], 0, 0, 0);
      }
    }
  };
  const int nt = N / C::KV;

  // ---- pass 1: (max, sum) of every query row ----
  float m[16], l[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    f32x16 sacc[2];
    scores(smem + cur * C::TILE, sacc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float mn = fmaxf(m[r], fmaxf(sacc[0][r], sacc[1][r]));
      l[r] = l[r] * __builtin_amdgcn_exp2f(m[r] - mn) + __builtin_amdgcn_exp2f(sacc[0][r] - mn) + __builtin_amdgcn_exp2f(sacc[1][r] - mn);
      m[r] = mn;
    }
    if (t + 1 < nt) store_tile(cur ^ 1);
    __syncthreads();
  }
  // the 32 lanes of one half wave hold the 32 key columns of the same 16 query rows
#pragma unroll
  for (int x = 1; x < 32; x <<= 1)
#pragma unroll
    for (int r = 0; r < 16; ++r) merge_ml(m[r], l[r], __shfl_xor(m[r], x), __shfl_xor(l[r], x));
#pragma unroll
  for (int r = 0; r < 16; ++r) l[r] = 1.0f / l[r];

  // ---- pass 2: probabilities ----
  float fsum = 0.f;  // FRAME: this lane's probability mass in the current key frame
  int tk_cur = 0;
  const int group = q0 >> 5;  // 32-row group of the wave
  auto flush = [&](int tk) {
    float v = fsum;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) v += __shfl_xor(v, x);
    if (lane == 0) out[((long)bh * (N / 32) + group) * T + tk] = v;
    fsum = 0.f;
  };
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    f32x16 sacc[2];
    scores(smem + cur * C::TILE, sacc);
    if constexpr (FULL) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* row = out + ((long)bh * N + q0 + (r & 3) + 8 * (r >> 2) + 4 * lh) * N + t * C::KV + lq;
        row[0] = __builtin_amdgcn_exp2f(sacc[0][r] - m[r]) * l[r];
        row[32] = __builtin_amdgcn_exp2f(sacc[1][r] - m[r]) * l[r];
      }
    } else {
      const int tk = t * C::KV / P;  // uniform over the workgroup
      if (tk != tk_cur) {
        flush(tk_cur);
        tk_cur = tk;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        fsum += (__builtin_amdgcn_exp2f(sacc[0][r] - m[r]) + __builtin_amdgcn_exp2f(sacc[1][r] - m[r])) * l[r];
    }
    if (t + 1 < nt) store_tile(cur ^ 1);
    __syncthreads();
  }
  if constexpr (!FULL) flush(tk_cur);
}

// out[o][e] = inv * sum_{g < G} part[o][g][e], g ascending
__global__ __launch_bounds__(256) void map_finalize_kernel(const float* __restrict__ part, float* __restrict__ out, long total, int G, int E, float inv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long o = i / E;
  const int e = (int)(i - o * E);
  float a = 0.f;
  for (int g = 0; g < G; ++g) a += part[(o * G + g) * E + e];
  out[i] = a * inv;
}

template <int CH>
struct MapChunkT;
template <>
struct MapChunkT<8> { typedef bf16x8 type; };
template <>
struct MapChunkT<4> { typedef bf16x4 type; };

constexpr int TM_PATCHES = 64;  // patch positions per workgroup of the temporal map kernel

// TT: compile-time bound of T (score registers); CH: bf16 elements per LDS / global access; PB: patch positions staged at a time
template <int TT, int CH>
__global__ __launch_bounds__(256) void attn_temporal_map_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k, float* __restrict__ part,
                                                                int T, int P, int heads, int d, int dstride, int PB) {
  typedef typename MapChunkT<CH>::type chunk_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int dl = d + 8;     // LDS row stride (elements), as attention_temporal.hip
  const int nch = d / CH;   // chunks per row
  const int rows = T * PB;  // rows of one operand: (t, pl)
  const int TT2 = T * T;
  bf16* sq = reinterpret_cast<bf16*>(smem);
  bf16* sk = sq + (long)rows * dl;
  float* sp = reinterpret_cast<float*>(sk + (long)rows * dl);  // [PB][T][T]; 2 * rows * dl * 2 bytes is a multiple of 16
  const int head = blockIdx.y, b = blockIdx.z;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // entries threadIdx.x + 256 u of the T x T sum (T <= 32)

  for (int c0 = 0; c0 < TM_PATCHES; c0 += PB) {
    const int p0 = blockIdx.x * TM_PATCHES + c0;
    const int total = 2 * rows * nch;
    for (int i = threadIdx.x; i < total; i += 256) {
      const int c = i % nch, r = (i / nch) % rows, w = i / (nch * rows);
      const int t = r / PB, pl = r % PB;
      const bf16* src = (w == 0 ? q : k) + ((((long)b * T + t) * heads + head) * P + p0 + pl) * dstride + c * CH;
      *reinterpret_cast<chunk_t*>(sq + ((long)w * rows + r) * dl + c * CH) = *reinterpret_cast<const chunk_t*>(src);
    }
    __syncthreads();
    // one thread per (pl, query frame): the forward's scores and exp2-domain softmax, the probabilities kept in fp32
    for (int item = threadIdx.x; item < rows; item += 256) {
      const int pl = item / T, qi = item % T;
      const bf16* qrow = sq + (long)(qi * PB + pl) * dl;
      float s[TT];
#pragma unroll
      for (int j = 0; j < TT; ++j) s[j] = 0.f;
      for (int c = 0; c < nch; ++c) {
        const chunk_t qc = *reinterpret_cast<const chunk_t*>(qrow + c * CH);
        float qv[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) qv[e] = bf2f(qc[e]);
#pragma unroll
        for (int j = 0; j < TT; ++j) {
          if (j < T) {
            const chunk_t kc = *reinterpret_cast<const chunk_t*>(sk + (long)(j * PB + pl) * dl + c * CH);
            float a = s[j];
#pragma unroll
            for (int e = 0; e < CH; ++e) a = fmaf(qv[e], bf2f(kc[e]), a);
            s[j] = a;
          }
        }
      }
      float mx = s[0];
#pragma unroll
      for (int j = 1; j < TT; ++j)
        if (j < T) mx = fmaxf(mx, s[j]);
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        if (j < T) {
          s[j] = exp2f(s[j] - mx);
          sum += s[j];
        }
      }
      const float inv = 1.0f / sum;
      float* prow = sp + (long)pl * TT2 + qi * T;
#pragma unroll
      for (int j = 0; j < TT; ++j)
        if (j < T) prow[j] = s[j] * inv;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = threadIdx.x + 256 * u;
      if (e < TT2)
        for (int pl = 0; pl < PB; ++pl) acc[u] += sp[(long)pl * TT2 + e];
    }
    __syncthreads();
  }
  float* dst = part + (((long)b * heads + head) * gridDim.x + blockIdx.x) * TT2;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = threadIdx.x + 256 * u;
    if (e < TT2) dst[e] = acc[u];
  }
}

template <int NT, int CH, bool ROPE>
__global__ __launch_bounds__(MA_THREADS) void matrix_attn_map_kernel(const bf16* __restrict__ z, const float* __restrict__ rope_cs,
                                                                     float* __restrict__ out, int L, int E, int h, int cc, int rr, float scale) {
  constexpr int TL = 16 * NT;
  __shared__ __attribute__((aligned(16))) float part[MA_WAVES][TL * TL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / (cc * rr), c = (blockIdx.x / rr) % cc, r = blockIdx.x % rr;
  const int hn = E / cc, hd = h / rr, R = hn * hd;
  const long ldz = 3L * h;
  const bf16* zb = z + (((long)b * L) * E + c * hn) * ldz + r * hd;  // q of (frame 0, n 0); frame stride E*ldz, n stride ldz
  const long lstride = (long)E * ldz;
  matrix_attn_scores<NT, CH, ROPE>(zb, rope_cs, lane, wave, L, h, hd, R, ldz, lstride, scale, part);
  if (threadIdx.x < L) {  // softmax over l', as the forward
    const float* row = part[0] + threadIdx.x * TL;
    float mx = row[0];
    for (int j = 1; j < L; ++j) mx = fmaxf(mx, row[j]);
    float sum = 0.f;
    for (int j = 0; j < L; ++j) sum += __expf(row[j] - mx);
    const float inv = 1.0f / sum;
    float* dst = out + ((long)blockIdx.x * L + threadIdx.x) * L;
    for (int j = 0; j < L; ++j) dst[j] = __expf(row[j] - mx) * inv;
  }
}

int launch_finalize(const float* part, float* out, long outer, int G, int E, float inv, hipStream_t s) {
  const long total = outer * E;
  hipLaunchKernelGGL(map_finalize_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, part, out, total, G, E, inv);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

template <int D, int DQK>
int launch_map_t(const bf16* q, const bf16* k, float* dst, bool full, int batch, int heads, int n, int patches, int tokens, hipStream_t s) {
  const dim3 grid(n / 128, batch * heads), blk(256);
  if (full)
    hipLaunchKernelGGL((attn_map_kernel<D, DQK, true>), grid, blk, 0, s, q, k, dst, n, patches, tokens);
  else
    hipLaunchKernelGGL((attn_map_kernel<D, DQK, false>), grid, blk, 0, s, q, k, dst, n, patches, tokens);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace

size_t attention_map_part_floats(int batch, int heads, int n, int tokens) { return (size_t)batch * heads * (n / 32) * tokens; }
size_t attention_temporal_map_part_floats(int batch, int heads, int tokens, int patches) {
  return (size_t)batch * heads * (patches / TM_PATCHES) * tokens * tokens;
}

int launch_attention_map(const bf16* q, const bf16* k, float* out, float* part, bool full, int batch, int heads, int n, int tokens, int d,
                         hipStream_t s) {
  DFOT_REQUIRE(q && k && out && (full || part), DFOT_ERR_ARG, "attention map: null pointer");
  DFOT_REQUIRE(batch > 0 && heads > 0 && (long)batch * heads <= 65535, DFOT_ERR_SHAPE, "attention map: batch %d, heads %d", batch, heads);
  DFOT_REQUIRE(d > 0 && d <= 128 && d % 4 == 0, DFOT_ERR_SHAPE, "attention map: head dim %d must be a multiple of 4, <= 128", d);
  DFOT_REQUIRE(n > 0 && n % 128 == 0, DFOT_ERR_SHAPE, "attention map: N=%d must be a multiple of 128", n);
  DFOT_REQUIRE(tokens >= 1 && tokens <= 32 && n % tokens == 0, DFOT_ERR_SHAPE, "attention map: %d frames must be 1 to 32 and divide N=%d", tokens, n);
  const int patches = n / tokens;
  DFOT_REQUIRE(patches % 64 == 0, DFOT_ERR_SHAPE, "attention map: %d patches per frame must be a multiple of 64", patches);
  float* dst = full ? out : part;
  int rc;
  if (d <= 32) rc = launch_map_t<64, 32>(q, k, dst, full, batch, heads, n, patches, tokens, s);
  else if (d <= 64) rc = launch_map_t<64, 64>(q, k, dst, full, batch, heads, n, patches, tokens, s);
  else if (d <= 80) rc = launch_map_t<128, 80>(q, k, dst, full, batch, heads, n, patches, tokens, s);
  else if (d <= 96) rc = launch_map_t<128, 96>(q, k, dst, full, batch, heads, n, patches, tokens, s);
  else rc = launch_map_t<128, 128>(q, k, dst, full, batch, heads, n, patches, tokens, s);
  if (rc || full) return rc;
  // F[bh][tq][tk] = (1/P) * sum over the P/32 row groups of frame tq
  return launch_finalize(part, out, (long)batch * heads * tokens, patches / 32, tokens, 1.0f / (float)patches, s);
}

int launch_attention_temporal_map(const bf16* q, const bf16* k, float* out, float* part, int batch, int tokens, int patches, int heads, int d,
                                  hipStream_t s) {
  DFOT_REQUIRE(q && k && out && part, DFOT_ERR_ARG, "temporal attention map: null pointer");
  DFOT_REQUIRE(batch > 0 && heads > 0 && batch <= 65535 && heads <= 65535, DFOT_ERR_SHAPE, "temporal attention map: batch %d, heads %d", batch, heads);
  DFOT_REQUIRE(tokens >= 1 && tokens <= 32, DFOT_ERR_SHAPE, "temporal attention map: %d frames (1 to 32 are supported)", tokens);
  DFOT_REQUIRE(d > 0 && d % 4 == 0 && d <= 128, DFOT_ERR_SHAPE, "temporal attention map: head dim %d must be a multiple of 4, <= 128", d);
  DFOT_REQUIRE(patches > 0 && patches % TM_PATCHES == 0, DFOT_ERR_SHAPE, "temporal attention map: %d patches per frame must be a multiple of %d",
               patches, TM_PATCHES);
  const int ch = d % 8 == 0 ? 8 : 4;
  const int dstride = attention_dstride(d);
  // PB patch positions staged at a time: the largest power of two whose q, k rows and T x T probabilities fit 48 KB of LDS (21.5 KB at
  // T = 32, d = 128 with PB = 1)
  const size_t per_p = (size_t)tokens * (2 * (d + 8) * sizeof(bf16) + tokens * sizeof(float));
  int pb = TM_PATCHES;
  while (pb > 1 && pb * per_p > 48 * 1024) pb >>= 1;
  const size_t lds = pb * per_p;
  const dim3 grid(patches / TM_PATCHES, heads, batch), blk(256);
#define LAUNCH(TT, CH) hipLaunchKernelGGL((attn_temporal_map_kernel<TT, CH>), grid, blk, lds, s, q, k, part, tokens, patches, heads, d, dstride, pb)
  const int tt = tokens <= 4 ? 4 : tokens <= 8 ? 8 : tokens <= 16 ? 16 : 32;
  if (ch == 8) {
    switch (tt) {
      case 4: LAUNCH(4, 8); break;
      case 8: LAUNCH(8, 8); break;
      case 16: LAUNCH(16, 8); break;
      default: LAUNCH(32, 8); break;
    }
  } else {
    switch (tt) {
      case 4: LAUNCH(4, 4); break;
      case 8: LAUNCH(8, 4); break;
      case 16: LAUNCH(16, 4); break;
      default: LAUNCH(32, 4); break;
    }
  }
#undef LAUNCH
  DFOT_CHECK_HIP(hipGetLastError());
  return launch_finalize(part, out, (long)batch * heads, patches / TM_PATCHES, tokens * tokens, 1.0f / (float)patches, s);
}

int launch_matrix_attn_map(const bf16* z, const float* rope_cs, float* out, int batch, int L, int E, int h, int cc, int rr, float scale,
                           hipStream_t s) {
  DFOT_REQUIRE(z && out, DFOT_ERR_ARG, "matrix attention map: null pointer");
  DFOT_REQUIRE(L >= 1 && L <= 32, DFOT_ERR_SHAPE, "matrix attention map: %d frame tokens (1 to 32 are supported)", L);
  DFOT_REQUIRE(batch > 0 && E > 0 && h > 0 && cc > 0 && rr > 0, DFOT_ERR_SHAPE, "matrix attention map: batch %d, E %d, h %d, heads (%d, %d)", batch, E,
               h, cc, rr);
  DFOT_REQUIRE(E % cc == 0, DFOT_ERR_SHAPE, "matrix attention map: embed_col_dim %d is not divisible by %d col heads", E, cc);
  DFOT_REQUIRE(h % rr == 0, DFOT_ERR_SHAPE, "matrix attention map: embed_row_dim %d is not divisible by %d row heads", h, rr);
  const int hd = h / rr;
  DFOT_REQUIRE(hd % 4 == 0, DFOT_ERR_SHAPE, "matrix attention map: row head dim %d must be a multiple of 4", hd);
  DFOT_REQUIRE((long)batch * cc * rr <= 0x7fffffffL && (long)(E / cc) * hd <= (1L << 26), DFOT_ERR_SHAPE,
               "matrix attention map: %ld problems of %ld entries", (long)batch * cc * rr, (long)(E / cc) * hd);
  const dim3 grid(batch * cc * rr), blk(MA_THREADS);
#define LAUNCH(NT, CH, ROPE) hipLaunchKernelGGL((matrix_attn_map_kernel<NT, CH, ROPE>), grid, blk, 0, s, z, rope_cs, out, L, E, h, cc, rr, scale)
#define PICK(NT, CH)         \
  if (rope_cs) {             \
    LAUNCH(NT, CH, true);    \
  } else {                   \
    LAUNCH(NT, CH, false);   \
  }
  if (L <= 16) {
    if (hd % 8 == 0) {
      PICK(1, 8)
    } else {
      PICK(1, 4)
    }
  } else {
    if (hd % 8 == 0) {
      PICK(2, 8)
    } else {
      PICK(2, 4)
    }
  }
#undef PICK
#undef LAUNCH
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace dfot

extern "C" {

size_t dfot_op_attention_map_workspace_bytes(int temporal, int batch, int heads, int tokens, int patches) {
  if (batch <= 0 || heads <= 0 || tokens <= 0 || patches <= 0) return 0;
  using namespace dfot;
  return sizeof(float) * (temporal ? attention_temporal_map_part_floats(batch, heads, tokens, patches)
                                   : attention_map_part_floats(batch, heads, tokens * patches, tokens));
}

int dfot_op_attention_map(const void* q, const void* k, void* out, void* workspace, size_t workspace_bytes, int form, int batch, int heads, int n,
                          int tokens, int d, void* stream) {
  using namespace dfot;
  DFOT_REQUIRE(form == DFOT_ATTN_MAP_FRAME || form == DFOT_ATTN_MAP_FULL, DFOT_ERR_ARG, "attention map: form %d unknown (0 = frame, 1 = full)", form);
  const bool full = form == DFOT_ATTN_MAP_FULL;
  if (!full && batch > 0 && heads > 0 && n > 0 && tokens > 0)
    DFOT_REQUIRE(workspace_bytes >= sizeof(float) * attention_map_part_floats(batch, heads, n, tokens), DFOT_ERR_SHAPE,
                 "attention map: workspace of %zu bytes, need %zu", workspace_bytes, sizeof(float) * attention_map_part_floats(batch, heads, n, tokens));
  return launch_attention_map((const bf16*)q, (const bf16*)k, (float*)out, (float*)workspace, full, batch, heads, n, tokens, d, (hipStream_t)stream);
}

int dfot_op_attention_temporal_map(const void* q, const void* k, void* out, void* workspace, size_t workspace_bytes, int batch, int tokens,
                                   int patches, int heads, int d, void* stream) {
  using namespace dfot;
  if (batch > 0 && heads > 0 && patches > 0 && tokens > 0)
    DFOT_REQUIRE(workspace_bytes >= sizeof(float) * attention_temporal_map_part_floats(batch, heads, tokens, patches), DFOT_ERR_SHAPE,
                 "temporal attention map: workspace of %zu bytes, need %zu", workspace_bytes,
                 sizeof(float) * attention_temporal_map_part_floats(batch, heads, tokens, patches));
  return launch_attention_temporal_map((const bf16*)q, (const bf16*)k, (float*)out, (float*)workspace, batch, tokens, patches, heads, d,
                                       (hipStream_t)stream);
}

int dfot_op_matrix_attention_map(const void* z, const float* rope_cs, void* out, int batch, int L, int E, int h, int cc, int rr, float scale,
                                 void* stream) {
  using namespace dfot;
  return launch_matrix_attn_map((const bf16*)z, rope_cs, (float*)out, batch, L, E, h, cc, rr, scale, (hipStream_t)stream);
}

}  // extern "C"
