// Backward of the temporal attention of the factorized-attention DiT (attention_temporal.hip): for every (video b, head, patch position p)
// the T <= 32 frames attend to each other, so one problem is a T x T score matrix over d <= 128 channels, and the whole of it -- scores,
// softmax, dP, dS -- is recomputed here from q, k, v and dO.  No log-sum-exp and no delta buffer come from the forward.
//
// Operands as the forward: q, k, v [frame][head][P][dstride] bf16 with q pre-scaled into the exp2 domain, dO compact
// [(video, frame, patch)][ldo].  dq, dk, dv use the layout of q, k, v (live columns only) under the contract of launch_attention_bwd:
// dq is the gradient of the UNSCALED q (factor 1/sqrt(d)), dk carries ln 2 (q holds log2 e).  qkv_grad_pack_kernel reads them as they are.
//
// Form: VALU, the forward's decomposition.  A workgroup owns PB consecutive p of one (b, head).
//   1. the d live columns of its q, k, v and dO rows go to LDS with 16-byte accesses (rows padded by 8 elements as in the forward);
//   A. one thread per (p, query frame i): s_j = <q_i, k_j> and dP_j = <dO_i, v_j> in fp32 registers, the forward's softmax (exp2 domain,
//      probabilities rounded to bf16, divided by the fp32 row sum), delta_i = sum_j P_ij dP_ij, dS_ij = P_ij (dP_ij - delta_i);
//      dq_i = sum_j dS_ij k_j leaves the thread chunk by chunk with 16-byte global stores (nothing in LDS is dead yet: q_i and dO_i are
//      read again in phase B by the threads of every key frame); the P and dS rows go to two fp32 LDS tiles [p][i][j], rows of TT + 1 words (TT: the compile-time bound of T)
//      so that the row writes of lanes i, i + 1, ... fall on different banks;
//   B. after a barrier one thread per (p, key frame j): dv_j = sum_i P_ij dO_i and dk_j = sum_i dS_ij q_i, read down the LDS columns
//      (lanes of adjacent j: adjacent words).  k and v are dead after phase A, so dk_j and dv_j overwrite the rows k_j and v_j;
//   2. after a barrier the workgroup stores those rows with 16-byte accesses.
// Every sum runs in a fixed order inside one thread, there are no atomics and no value crosses a workgroup: a video gives the same bits
// alone, in a batch and on repeat.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace dfot {
namespace {

constexpr int CH = 8;  // bf16 elements per LDS / global access
constexpr int FG = 4;  // frames per predicated group

// acc += a * b as one instruction the vectorizer cannot see.  Written with fmaf, the eight channel FMAs that share one probability (or
// the FG frame FMAs that share one q channel) are packed into v_pk_fma_f32 with the shared factor splatted over eight registers, and
// the splats of all TT frames are hoisted out of the channel loop: 8 x 2 x 32 VGPRs at TT = 32, which spills.
__device__ __forceinline__ void fmac(float& acc, float a, float b) { asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b)); }

// TT: compile-time bound of T (the registers of the T-wide fp32 rows).  The frame loops are fully unrolled in groups of FG frames: a
// group runs when its first frame is below the run-time T (a uniform branch), and inside a running group a frame >= T reads the rows of
// frame T - 1 and is masked out of the result (score -inf -> P = dS = 0), so there is no branch per frame and no read outside the T
// staged rows.
template <int TT>
__global__ __launch_bounds__(256) void attention_temporal_bwd_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                                     const bf16* __restrict__ v, const bf16* __restrict__ d_o, long ldo,
                                                                     bf16* __restrict__ dq, bf16* __restrict__ dk, bf16* __restrict__ dv,
                                                                     int T, int P, int heads, int d, int dstride, int PB, float sq,
                                                                     float sk_scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int ts = TT + 1;     // row stride (words) of the P / dS tiles: odd
  const int dl = d + 8;          // LDS row stride (elements)
  const int nch = d / CH;        // chunks per row
  const int rows = T * PB;       // rows of one operand: (t, pl)
  const int fstep = PB * dl;     // elements from frame t to frame t + 1 of one p
  bf16* sq_ = reinterpret_cast<bf16*>(smem);
  bf16* sk = sq_ + rows * dl;
  bf16* sv = sk + rows * dl;
  bf16* sdo = sv + rows * dl;
  float* sp = reinterpret_cast<float*>(sdo + rows * dl);  // 4 * rows * dl * 2 bytes: a multiple of 16
  float* sds = sp + PB * T * ts;
  const int p0 = blockIdx.x * PB, head = blockIdx.y, b = blockIdx.z;

  // 1. global -> LDS.  row r = t * PB + pl; q / k / v row ((b*T + t) * heads + head) * P + p0 + pl, dO row (b*T + t) * P + p0 + pl
  const int total = 4 * rows * nch;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int c = i % nch, r = (i / nch) % rows, w = i / (nch * rows);
    const int t = r / PB, pl = r % PB;
    const bf16* src = w == 3 ? d_o + (((long)b * T + t) * P + p0 + pl) * ldo + (long)head * d + c * CH
                             : (w == 0 ? q : w == 1 ? k : v) + ((((long)b * T + t) * heads + head) * P + p0 + pl) * dstride + c * CH;
    *reinterpret_cast<bf16x8*>(sq_ + (w * rows + r) * dl + c * CH) = *reinterpret_cast<const bf16x8*>(src);
  }
  __syncthreads();

  // A. one thread per (pl, i); lanes of one p are adjacent so that their k / v reads are LDS broadcasts
#pragma unroll 1
  for (int item = threadIdx.x; item < rows; item += blockDim.x) {
    const int pl = item / T, qi = item % T;
    const bf16* qrow = sq_ + (qi * PB + pl) * dl;
    const bf16* orow = sdo + (qi * PB + pl) * dl;
    float s[TT], dp[TT];
#pragma unroll
    for (int j = 0; j < TT; ++j) s[j] = 0.f, dp[j] = 0.f;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
      const bf16x8 qc = *reinterpret_cast<const bf16x8*>(qrow + c * CH);
      const bf16x8 oc = *reinterpret_cast<const bf16x8*>(orow + c * CH);
      float qf[CH], of[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) qf[e] = bf2f(qc[e]), of[e] = bf2f(oc[e]);
      const int col = pl * dl + c * CH;
#pragma unroll
      for (int g = 0; g < TT; g += FG) {
        if (g < T) {
#pragma unroll
          for (int j = g; j < g + FG; ++j) {
            const int off = min(j, T - 1) * fstep + col;
            const bf16x8 kc = *reinterpret_cast<const bf16x8*>(sk + off);
            const bf16x8 vc = *reinterpret_cast<const bf16x8*>(sv + off);
            float a = s[j], gd = dp[j];
#pragma unroll
            for (int e = 0; e < CH; ++e) fmac(a, qf[e], bf2f(kc[e])), fmac(gd, of[e], bf2f(vc[e]));
            s[j] = a, dp[j] = gd;
          }
        }
      }
    }
    float mx = s[0];
#pragma unroll
    for (int j = 1; j < TT; ++j) {
      s[j] = j < T ? s[j] : -INFINITY;  // frames past T: P = 0, dS = 0
      mx = fmaxf(mx, s[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const float pj = exp2f(s[j] - mx);
      sum += pj;
      s[j] = bf2f(f2bf(pj));  // the forward's P.V takes bf16 probabilities
    }
    const float inv = 1.0f / sum;
    float delta = 0.f;
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      s[j] *= inv;
      delta = fmaf(s[j], dp[j], delta);
    }
    float* prow = sp + (pl * T + qi) * ts;
    float* dsrow = sds + (pl * T + qi) * ts;
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      dp[j] = s[j] * (dp[j] - delta);  // dS_ij
      prow[j] = s[j];
      dsrow[j] = dp[j];
    }
    bf16* dqrow = dq + ((((long)b * T + qi) * heads + head) * P + p0 + pl) * dstride;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
      float acc[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) acc[e] = 0.f;
      const int col = pl * dl + c * CH;
#pragma unroll
      for (int g = 0; g < TT; g += FG) {
        if (g < T) {
#pragma unroll
          for (int j = g; j < g + FG; ++j) {
            const bf16x8 kc = *reinterpret_cast<const bf16x8*>(sk + min(j, T - 1) * fstep + col);
#pragma unroll
            for (int e = 0; e < CH; ++e) fmac(acc[e], dp[j], bf2f(kc[e]));
          }
        }
      }
      bf16x8 out;
#pragma unroll
      for (int e = 0; e < CH; ++e) out[e] = f2bf(acc[e] * sq);
      *reinterpret_cast<bf16x8*>(dqrow + c * CH) = out;
    }
  }
  __syncthreads();

  // B. one thread per (pl, j): the columns j of P and dS; dk_j / dv_j replace k_j / v_j (dead since the barrier)
#pragma unroll 1
  for (int item = threadIdx.x; item < rows; item += blockDim.x) {
    const int pl = item / T, kj = item % T;
    const float* pcol = sp + pl * T * ts + kj;
    const float* dscol = sds + pl * T * ts + kj;
    float pc[TT], dsc[TT];
#pragma unroll
    for (int i = 0; i < TT; ++i) {
      const int r = min(i, T - 1) * ts;
      const float a = pcol[r], g = dscol[r];
      pc[i] = i < T ? a : 0.f, dsc[i] = i < T ? g : 0.f;
    }
    bf16* krow = sk + (kj * PB + pl) * dl;
    bf16* vrow = sv + (kj * PB + pl) * dl;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
      float ak[CH], av[CH];
#pragma unroll
      for (int e = 0; e < CH; ++e) ak[e] = 0.f, av[e] = 0.f;
      const int col = pl * dl + c * CH;
#pragma unroll
      for (int g = 0; g < TT; g += FG) {
        if (g < T) {
#pragma unroll
          for (int i = g; i < g + FG; ++i) {
            const int off = min(i, T - 1) * fstep + col;
            const bf16x8 qc = *reinterpret_cast<const bf16x8*>(sq_ + off);
            const bf16x8 oc = *reinterpret_cast<const bf16x8*>(sdo + off);
#pragma unroll
            for (int e = 0; e < CH; ++e) fmac(ak[e], dsc[i], bf2f(qc[e])), fmac(av[e], pc[i], bf2f(oc[e]));
          }
        }
      }
      bf16x8 ko, vo;
#pragma unroll
      for (int e = 0; e < CH; ++e) ko[e] = f2bf(ak[e] * sk_scale), vo[e] = f2bf(av[e]);
      *reinterpret_cast<bf16x8*>(krow + c * CH) = ko;
      *reinterpret_cast<bf16x8*>(vrow + c * CH) = vo;
    }
  }
  __syncthreads();

  // 2. LDS -> global: row (t, pl) of dk / dv -> [((b*T + t) * heads + head) * P + p0 + pl][0 .. d)
  for (int i = threadIdx.x; i < 2 * rows * nch; i += blockDim.x) {
    const int c = i % nch, r = (i / nch) % rows, w = i / (nch * rows);
    const int t = r / PB, pl = r % PB;
    *reinterpret_cast<bf16x8*>((w == 0 ? dk : dv) + ((((long)b * T + t) * heads + head) * P + p0 + pl) * dstride + c * CH) =
        *reinterpret_cast<const bf16x8*>((w == 0 ? sk : sv) + r * dl + c * CH);
  }
}

}  // namespace

int launch_attention_temporal_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dq, bf16* dk, bf16* dv,
                                  int batch, int tokens, int patches, int heads, int d, hipStream_t s) {
  DFOT_REQUIRE(q && k && v && d_o && dq && dk && dv, DFOT_ERR_ARG, "temporal attention backward: null pointer");
  DFOT_REQUIRE(batch > 0 && heads > 0 && batch <= 65535 && heads <= 65535, DFOT_ERR_SHAPE, "temporal attention backward: batch %d, heads %d",
               batch, heads);
  DFOT_REQUIRE(tokens >= 1 && tokens <= 32, DFOT_ERR_SHAPE, "temporal attention backward: %d frames (1 to 32 are supported)", tokens);
  DFOT_REQUIRE(d > 0 && d % 8 == 0 && d <= 128, DFOT_ERR_SHAPE, "temporal attention backward: head dim %d must be a multiple of 8, <= 128", d);
  // (the grid is patches / pb with pb a power of two <= 32)
  DFOT_REQUIRE(patches > 0 && patches % 64 == 0, DFOT_ERR_SHAPE, "temporal attention backward: %d patches per frame must be a multiple of 64",
               patches);
  DFOT_REQUIRE(ldo >= (long)heads * d && ldo % 8 == 0, DFOT_ERR_SHAPE,
               "temporal attention backward: ldo %ld must cover %d columns and be a multiple of 8", ldo, heads * d);
  const int dstride = attention_dstride(d);
  const int tt = tokens <= 4 ? 4 : tokens <= 8 ? 8 : tokens <= 16 ? 16 : 32;  // the kernel's compile-time bound of T
  // PB consecutive patch positions per workgroup, sized as the forward sizes it: the largest power of two whose four staged operands
  // and two T x (TT + 1) fp32 tiles fit 40 KB of LDS; 42.25 KB at T = 32, d = 128 with PB = 1 (below the 64 KB a launch may ask for)
  const size_t per_p = (size_t)4 * tokens * (d + 8) * sizeof(bf16) + (size_t)2 * tokens * (tt + 1) * sizeof(float);
  int pb = 32;
  while (pb > 1 && pb * per_p > 40 * 1024) pb >>= 1;
  const size_t lds = pb * per_p;
  const int threads = std::min(256, std::max(64, (pb * tokens + 63) / 64 * 64));
  const dim3 grid(patches / pb, heads, batch), blk(threads);
  const float sq = 1.0f / sqrtf((float)d), sk = 0.6931471805599453f;  // as launch_attention_bwd
#define LAUNCH(TT)                                                                                                                       \
  hipLaunchKernelGGL((attention_temporal_bwd_kernel<TT>), grid, blk, lds, s, q, k, v, d_o, ldo, dq, dk, dv, tokens, patches, heads, d, \
                     dstride, pb, sq, sk)
  switch (tt) {
    case 4: LAUNCH(4); break;
    case 8: LAUNCH(8); break;
    case 16: LAUNCH(16); break;
    default: LAUNCH(32); break;
  }
#undef LAUNCH
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace dfot

extern "C" int dfot_op_attention_temporal_bwd(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dq, void* dk,
                                              void* dv, int batch, int tokens, int patches, int heads, int d, void* stream) {
  using namespace dfot;
  // the op keeps its documented contract (dfot_hip.h); the launcher itself also takes the engine's 64-patch frames
  DFOT_REQUIRE(patches > 0 && patches % 128 == 0, DFOT_ERR_SHAPE, "temporal attention backward: %d patches per frame must be a multiple of 128",
               patches);
  return launch_attention_temporal_bwd((const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, ldo, (bf16*)dq, (bf16*)dk, (bf16*)dv,
                                       batch, tokens, patches, heads, d, (hipStream_t)stream);
}

// the same launcher at 64 patches per frame, the shape the FacDiT trainer runs it at for the res-128 recipes; any 1 <= tokens <= 32 (that
// a training window is a whole number of 128-row tiles is the engine's rule, not this kernel's)
extern "C" int dfot_op_attention_temporal_bwd_p64(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dq, void* dk,
                                                  void* dv, int batch, int tokens, int heads, int d, void* stream) {
  using namespace dfot;
  return launch_attention_temporal_bwd((const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, ldo, (bf16*)dq, (bf16*)dk, (bf16*)dv,
                                       batch, tokens, 64, heads, d, (hipStream_t)stream);
}
