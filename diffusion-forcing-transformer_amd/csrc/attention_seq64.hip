// Non-causal self-attention over sequences of exactly 64 tokens (gfx950): the per-frame spatial attention of FacDiT / FacMatDiT at 64
// patches per frame (the taichi res-128 recipes: KL-f8 latents 4x16x16, patch 2).  launch_attention_padded's kernels own 128 query rows of
// ONE sequence and so cannot run it.
//
// One workgroup = 2 waves = the 64 query rows of ONE (sequence, head); each wave owns 32 query rows.  The whole K and V of the sequence
// are one 64-key tile (AttnCfg<D>: 8 or 16 KB each), so the softmax is single-pass: no key loop, no running max, no rescale.
//   S^T (keys x q) = K   (A operand, LDS rows)             x Q^T (B operand, registers)
//   O^T (dv   x q) = V^T (A operand, LDS transposed read)  x P^T (B operand = the exp'd S^T registers)
// as in attention.hip (whose header has the operand layouts): the query index stays on the MFMA lane, so the row max and the row sum are
// lane-local apart from one exchange with lane ^ 32.  The K / V image in LDS and the V^T fragment are those of attention_common.h.
// Scores are in the exp2 domain: the caller folds log2(e)/sqrt(d) into q.
//
// Rows a work item does not own: every global address of a workgroup is inside its own (sequence, head) -- 64 rows of q, k, v at
// ((seq * heads + head) * 64) * D, and output rows seq * 64 .. seq * 64 + 63, columns head * d .. head * d + d - 1.  There is no packing
// of two sequences into a tile and therefore no tail case: the grid is exactly nseq * heads workgroups, and the operand buffers need no
// slack behind the last sequence.  The summation order is fixed by (D, DQK, DV), i.e. by d alone: a sequence's bits do not depend on the
// launch it is part of.  No atomics, no allocation, no synchronisation with the host.
#include "attention_common.h"
#include "dfot_hip.h"
#include "kernels.h"

namespace dfot {
namespace {

// D: row stride of q / k / v (64 or 128); DQK / DV: head-dim columns actually multiplied (multiples of 16 / 32 covering d; the pad
// columns d..DQK, d..DV hold zeros); d: live output columns (a multiple of 8)
template <int D, int DQK, int DV>
__global__ __launch_bounds__(128) void attn_seq64_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                         const bf16* __restrict__ V, bf16* __restrict__ O, long ldo, int heads, int d) {
  static_assert(DQK % 16 == 0 && DV % 32 == 0 && DQK <= D && DV <= D, "head-dim sub-range");
  using C = AttnCfg<D>;
  constexpr int KCH = DQK / 8, VCH = DV / 8;  // live 16-byte chunks per K / V row
  constexpr int KPT = 64 * KCH / 128, VPT = 64 * VCH / 128;  // chunks per thread
  __shared__ __attribute__((aligned(16))) char smem[2 * C::TILE];
  char* sk = smem;
  char* sv = smem + C::TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int bh = blockIdx.x;  // (sequence, head)
  const long base = (long)bh * 64 * D;
  const bf16* Qb = Q + base;
  const bf16* Kb = K + base;
  const bf16* Vb = V + base;
  const int q0 = wave * 32;

  // global -> registers: the live chunks of K and V (all loads in flight together), then this lane's Q fragments
  bf16x8 rk[KPT], rv[VPT];
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int e = tid + 128 * i;
    rk[i] = *reinterpret_cast<const bf16x8*>(Kb + (e / KCH) * D + (e % KCH) * 8);
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int e = tid + 128 * i;
    rv[i] = *reinterpret_cast<const bf16x8*>(Vb + (e / VCH) * D + (e % VCH) * 8);
  }
  // Q fragments: B operand, lane holds Q[q0+lq][16*ks + 8*lh + j]
  bf16x8 qf[DQK / 16];
#pragma unroll
  for (int ks = 0; ks < DQK / 16; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(Qb + (q0 + lq) * D + ks * 16 + lh * 8);

  // registers -> LDS in the swizzled image (the dead chunk positions of a row are neither written nor read)
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int e = tid + 128 * i;
    const int row = e / KCH, c = e % KCH;
    *reinterpret_cast<bf16x8*>(sk + row * C::ROWB + C::swz_k(row, c) * 16) = rk[i];
  }
#pragma unroll
  for (int i = 0; i < VPT; ++i) {
    const int e = tid + 128 * i;
    const int row = e / VCH, c = e % VCH;
    *reinterpret_cast<bf16x8*>(sv + row * C::ROWB + C::swz_v(row, c) * 16) = rv[i];
  }
  __syncthreads();

  // ---- S^T = K Q^T : two 32-key sub-tiles; lane holds 16 + 16 keys of query column lq, lane ^ 32 the other 32 ----
  f32x16 sacc[2];
#pragma unroll
  for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[kt2][r] = 0.f;
    const int row = kt2 * 32 + lq;
#pragma unroll
    for (int ks = 0; ks < DQK / 16; ++ks) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + row * C::ROWB + C::swz_k(row, ks * 2 + lh) * 16);
      sacc[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc[kt2], 0, 0, 0);
    }
  }

  // ---- single-pass softmax over the 64 keys (exp2 domain, fp32) ----
  float mx = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
  for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sacc[0][r]), sacc[1][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float rs = 0.f;
  bf16x8 pf[2][2];
#pragma unroll
  for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(sacc[kt2][8 * s + j] - mx);
        rs += p;
        pf[kt2][s][j] = f2bf(p);
      }
  const float inv = 1.0f / (rs + __shfl_xor(rs, 32));

  // ---- O^T = V^T P^T ----
  f32x16 oacc[DV / 32];
#pragma unroll
  for (int dvt = 0; dvt < DV / 32; ++dvt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dvt][r] = 0.f;
#pragma unroll
    for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_v<D>(sv, dvt, kt2, s, lane), pf[kt2][s], oacc[dvt], 0, 0, 0);
  }

  // ---- normalise and store.  The lane holds O[q0+lq][dvt*32 + 8*g + 4*lh + {0..3}] in oacc[dvt][4g..4g+3]; for every pair of groups
  // (g = 2a, 2a+1) the two lanes of a query row swap one 4-column half, after which lane lh owns the 8 consecutive columns
  // dvt*32 + 16*a + 8*lh .. +7: one 16-byte store per lane, and only where those columns are live (d % 8 == 0: all or none) ----
  bf16* orow = O + ((long)(bh / heads) * 64 + q0 + lq) * ldo + (long)(bh % heads) * d;
#pragma unroll
  for (int dvt = 0; dvt < DV / 32; ++dvt)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      bf16x4 keep, give;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16 lo = f2bf(oacc[dvt][8 * a + j] * inv), hi = f2bf(oacc[dvt][8 * a + 4 + j] * inv);
        keep[j] = lh ? hi : lo;
        give[j] = lh ? lo : hi;
      }
      u32x2 w = __builtin_bit_cast(u32x2, give);
      w[0] = (unsigned)__shfl_xor((int)w[0], 32);
      w[1] = (unsigned)__shfl_xor((int)w[1], 32);
      const bf16x4 got = __builtin_bit_cast(bf16x4, w);
      const bf16x4 c0 = lh ? got : keep, c1 = lh ? keep : got;  // columns +0..3, +4..7
      const int c = dvt * 32 + 16 * a + 8 * lh;
      if (c < d) *reinterpret_cast<bf16x8*>(orow + c) = bf16x8{c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    }
}

template <int D, int DQK, int DV>
int launch_seq64(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int nseq, int heads, int d, hipStream_t stream) {
  hipLaunchKernelGGL((attn_seq64_kernel<D, DQK, DV>), dim3(nseq * heads), dim3(128), 0, stream, q, k, v, o, ldo, heads, d);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace

// q, k, v [nseq][heads][64][attention_dstride(d)] as launch_attention_padded takes them with n = 64 (pad columns zero, q in the exp2
// domain); o compact: o[(seq*64 + row)][head*d + c], c < d, row stride ldo
int launch_attention_seq64(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int nseq, int heads, int d, hipStream_t stream) {
  DFOT_REQUIRE(q && k && v && o, DFOT_ERR_ARG, "attention_seq64: null pointer");
  DFOT_REQUIRE(d > 0 && d <= 128 && d % 8 == 0, DFOT_ERR_SHAPE, "attention_seq64: head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(nseq > 0 && heads > 0 && (long)nseq * heads <= 0x7fffffffL, DFOT_ERR_SHAPE, "attention_seq64: %d sequences, %d heads", nseq, heads);
  DFOT_REQUIRE(ldo >= (long)heads * d && ldo % 8 == 0, DFOT_ERR_SHAPE,
               "attention_seq64: output row stride %ld must cover %d columns and be a multiple of 8 (16-byte stores)", ldo, heads * d);
  if (d <= 32) return launch_seq64<64, 32, 32>(q, k, v, o, ldo, nseq, heads, d, stream);
  if (d <= 64) return launch_seq64<64, 64, 64>(q, k, v, o, ldo, nseq, heads, d, stream);
  if (d <= 80) return launch_seq64<128, 80, 96>(q, k, v, o, ldo, nseq, heads, d, stream);
  if (d <= 96) return launch_seq64<128, 96, 96>(q, k, v, o, ldo, nseq, heads, d, stream);
  return launch_seq64<128, 128, 128>(q, k, v, o, ldo, nseq, heads, d, stream);
}

}  // namespace dfot

extern "C" int dfot_op_attention_seq64(const void* q, const void* k, const void* v, void* o, int ldo, int nseq, int heads, int d, void* stream) {
  using namespace dfot;
  return launch_attention_seq64((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, ldo, nseq, heads, d, (hipStream_t)stream);
}
