// Temporal attention of the factorized-attention DiT (dit_base.py:405-413): for every (video b, head, patch position p) the T frames
// b*T .. b*T+T-1 attend to each other at that p.  T <= 32, so one problem is a T x T score matrix over d <= 128 channels.
//
// Operands are read where the QKV epilogue left them for the per-frame spatial block ([frame][head][P][dstride] bf16, q pre-scaled
// into the exp2 domain); the "(b t) p -> (b p) t" regrouping of the reference is addressing only.  A workgroup owns PB consecutive p of
// one (b, head): for each of the T frames that is PB adjacent rows in memory, and its output is PB adjacent d-wide row segments per frame.
//
// Form: VALU.  The kernel moves (3 dstride + d) * 2 bytes per (row, head) for 4 T d flop -- 0.1 to 2.5 flop per byte for T in 1..32 --
// so it is bound by memory, not by the matrix pipe, and MFMA tiles would be mostly padding (T = 3 or 5 in a 16-wide tile).
//   1. the workgroup copies the d live columns of its q, k, v rows into LDS with 16-byte accesses (rows padded by 8 elements: the 16-byte
//      reads of step 2 by lanes of different p then fall on different banks, lanes of the same p read the same address -> broadcast);
//   2. one thread per (p, query frame i): scores s[j] = <q_i, k_j> in fp32 registers, softmax in the exp2 domain (fp32), the
//      probabilities rounded to bf16, o_i = sum_j p_j v_j accumulated in fp32 and divided by the fp32 row sum;
//   3. o_i overwrites q_i in LDS (only this thread read it); after a barrier the workgroup stores the rows with 16-byte accesses.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace dfot {
namespace {

template <int CH>
struct ChunkT;
template <>
struct ChunkT<8> { typedef bf16x8 type; };
template <>
struct ChunkT<4> { typedef bf16x4 type; };

// TT: compile-time bound of T (score registers); CH: bf16 elements per LDS / global access (8 when d % 8 == 0, else 4)
template <int TT, int CH>
__global__ __launch_bounds__(256) void attention_temporal_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                                 const bf16* __restrict__ v, bf16* __restrict__ o, long ldo, int T,
                                                                 int P, int heads, int d, int dstride, int PB) {
  typedef typename ChunkT<CH>::type chunk_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int dl = d + 8;          // LDS row stride (elements)
  const int nch = d / CH;        // chunks per row
  const int rows = T * PB;       // rows of one operand: (t, pl)
  bf16* sq = reinterpret_cast<bf16*>(smem);
  bf16* sk = sq + (long)rows * dl;
  bf16* sv = sk + (long)rows * dl;
  const int p0 = blockIdx.x * PB, head = blockIdx.y, b = blockIdx.z;

  // 1. global -> LDS.  row r = t * PB + pl; source row ((b*T + t) * heads + head) * P + p0 + pl
  const int total = 3 * rows * nch;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int c = i % nch, r = (i / nch) % rows, w = i / (nch * rows);
    const int t = r / PB, pl = r % PB;
    const bf16* src = (w == 0 ? q : w == 1 ? k : v) + ((((long)b * T + t) * heads + head) * P + p0 + pl) * dstride + c * CH;
    *reinterpret_cast<chunk_t*>(sq + ((long)w * rows + r) * dl + c * CH) = *reinterpret_cast<const chunk_t*>(src);
  }
  __syncthreads();

  // 2. one thread per (pl, i); lanes of one p are adjacent so that their k / v reads are LDS broadcasts
  for (int item = threadIdx.x; item < rows; item += blockDim.x) {
    const int pl = item / T, qi = item % T;
    bf16* qrow = sq + (long)(qi * PB + pl) * dl;
    float s[TT];
#pragma unroll
    for (int j = 0; j < TT; ++j) s[j] = 0.f;
    for (int c = 0; c < nch; ++c) {
      const chunk_t qc = *reinterpret_cast<const chunk_t*>(qrow + c * CH);
      float qf[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) qf[e] = bf2f(qc[e]);
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        if (j < T) {
          const chunk_t kc = *reinterpret_cast<const chunk_t*>(sk + (long)(j * PB + pl) * dl + c * CH);
          float a = s[j];
#pragma unroll
          for (int e = 0; e < CH; ++e) a = fmaf(qf[e], bf2f(kc[e]), a);
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
        const float pj = exp2f(s[j] - mx);
        sum += pj;
        s[j] = bf2f(f2bf(pj));  // P.V takes bf16 operands
      }
    }
    const float inv = 1.0f / sum;
    for (int c = 0; c < nch; ++c) {
      float acc[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) acc[e] = 0.f;
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        if (j < T) {
          const chunk_t vc = *reinterpret_cast<const chunk_t*>(sv + (long)(j * PB + pl) * dl + c * CH);
#pragma unroll
          for (int e = 0; e < CH; ++e) acc[e] = fmaf(s[j], bf2f(vc[e]), acc[e]);
        }
      }
      chunk_t oc;
#pragma unroll
      for (int e = 0; e < CH; ++e) oc[e] = f2bf(acc[e] * inv);
      *reinterpret_cast<chunk_t*>(qrow + c * CH) = oc;  // 3. this thread's q row is dead: it carries the output row
    }
  }
  __syncthreads();

  // LDS -> global: row (t, pl) -> o[((b*T + t) * P + p0 + pl)][head*d ...]
  for (int i = threadIdx.x; i < rows * nch; i += blockDim.x) {
    const int c = i % nch, r = i / nch;
    const int t = r / PB, pl = r % PB;
    *reinterpret_cast<chunk_t*>(o + (((long)b * T + t) * P + p0 + pl) * ldo + (long)head * d + c * CH) =
        *reinterpret_cast<const chunk_t*>(sq + (long)r * dl + c * CH);
  }
}

}  // namespace

int launch_attention_temporal(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int tokens, int patches, int heads,
                              int d, hipStream_t s) {
  DFOT_REQUIRE(q && k && v && o, DFOT_ERR_ARG, "temporal attention: null pointer");
  DFOT_REQUIRE(batch > 0 && heads > 0 && batch <= 65535 && heads <= 65535, DFOT_ERR_SHAPE, "temporal attention: batch %d, heads %d", batch, heads);
  DFOT_REQUIRE(tokens >= 1 && tokens <= 32, DFOT_ERR_SHAPE, "temporal attention: %d frames (1 to 32 are supported)", tokens);
  DFOT_REQUIRE(d > 0 && d % 4 == 0 && d <= 128, DFOT_ERR_SHAPE, "temporal attention: head dim %d must be a multiple of 4, <= 128", d);
  // (the grid is patches / pb with pb a power of two <= 32)
  DFOT_REQUIRE(patches > 0 && patches % 64 == 0, DFOT_ERR_SHAPE, "temporal attention: %d patches per frame must be a multiple of 64", patches);
  const int ch = d % 8 == 0 ? 8 : 4;
  DFOT_REQUIRE(ldo >= (long)heads * d && ldo % ch == 0, DFOT_ERR_SHAPE, "temporal attention: ldo %ld must cover %d columns and be a multiple of %d",
               ldo, heads * d, ch);
  const int dstride = attention_dstride(d);
  // PB consecutive patch positions per workgroup: the largest power of two whose q, k, v rows fit 40 KB of LDS (several workgroups per
  // CU stay resident, so one's loads overlap another's arithmetic); 26 KB at T = 32, d = 128 with PB = 1
  const size_t per_p = (size_t)3 * tokens * (d + 8) * sizeof(bf16);
  int pb = 32;
  while (pb > 1 && pb * per_p > 40 * 1024) pb >>= 1;
  const size_t lds = pb * per_p;
  const int threads = std::min(256, std::max(64, (pb * tokens + 63) / 64 * 64));
  const dim3 grid(patches / pb, heads, batch), blk(threads);
#define LAUNCH(TT, CH) \
  hipLaunchKernelGGL((attention_temporal_kernel<TT, CH>), grid, blk, lds, s, q, k, v, o, ldo, tokens, patches, heads, d, dstride, pb)
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
  return DFOT_OK;
}

}  // namespace dfot

extern "C" int dfot_op_attention_temporal(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int tokens, int patches,
                                          int heads, int d, void* stream) {
  using namespace dfot;
  // the op keeps its documented contract (dfot_hip.h); the launcher itself also takes the engine's 64-patch frames
  DFOT_REQUIRE(patches > 0 && patches % 128 == 0, DFOT_ERR_SHAPE, "temporal attention: %d patches per frame must be a multiple of 128", patches);
  return launch_attention_temporal((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, ldo, batch, tokens, patches, heads, d,
                                   (hipStream_t)stream);
}
