// Backward of the non-causal self-attention over sequences of exactly 64 tokens (attention_seq64.hip): the per-frame spatial attention of
// FacDiT / FacMatDiT at 64 patches per frame (the taichi res-128 recipes).  launch_attention_bwd's kernels own 128 rows of ONE sequence
// and so cannot run it.
//
// Operands as the forward: q, k, v [nseq][heads][64][dstride] bf16, pad columns zero, q pre-scaled into the exp2 domain; dO compact
// [(seq*64 + row)][ldo], head hd at column hd*d.  dq, dk, dv use the layout of q, k, v (live columns c < d only: with d % 8 == 0 every
// 16-byte store is all-live or all-pad, pad columns are never written) under the contract of launch_attention_bwd: dq is the gradient of
// the UNSCALED q (factor 1/sqrt(d)), dk carries ln 2 (q holds log2 e).
//
// The whole problem of one (sequence, head) is ONE 64 x 64 score tile, so nothing comes from the forward: no log-sum-exp, no delta
// pre-pass, no o.  The single-pass softmax (row max, row sum) is recomputed from q and k as attention_temporal_bwd.hip does for its T x T
// problem, and delta[q] = sum_j P[q][j] dP[q][j] is formed in the kernel.  P = exp2(S' - max) / sum in fp32, dS = P o (dP - delta) in fp32;
// P and dS are rounded to bf16 as MFMA operands.
//
// One workgroup = 4 waves = one (sequence, head).  Q, K, V and dO are staged once as 64-row tiles in LDS, rows padded by 16 bytes as in
// attention_bwd.hip so that one layout serves row reads (ds_read_b128) and transposed reads (ds_read_b64_tr_b16); the dO chunks at or
// beyond column d (the next head / padding of the compact layout) are staged as zeros.  Every product keeps its reduction index on MFMA
// registers and its output index on the lanes (v_mfma_f32_32x32x16_bf16, operand layouts in attention_bwd.hip), so S and dP are computed
// in both orientations, 8 tile GEMMs instead of 5, and neither P nor dS is transposed through LDS:
//   waves 0, 1 (query on lane, 32 queries each): S^T = K Q^T, dP^T = V dO^T, the row statistics, dS^T, dQ^T = K^T dS^T;
//   waves 2, 3 (key on lane, 32 keys each):      S = Q K^T,   dP = dO V^T,   P, dS, dV^T = dO^T P, dK^T = Q^T dS.
// With the query on the lane the row max, the row sum and delta are lane-local apart from one exchange with lane ^ 32; waves 0, 1 leave
// them in LDS (-max, 1/sum, delta: 3 x 64 floats, row = query) and waves 2, 3 read them behind one barrier, four rows per 16-byte read,
// in the order of their accumulator registers.  The role is wave-uniform (a scalar branch), so EXEC is full at every transposed read, and
// the S / dP products of the two roles are one piece of code on swapped tiles.
// Why four waves with two per role, not two waves doing both: waves 2, 3 multiply their S and dP (half of their MFMAs) while waves 0, 1
// reduce the statistics, so only the softmax of 32 rows stands in front of the barrier; a wave holds the accumulators of one role only
// (at d = 128 dK and dV alone are 128 registers); and the four waves of the single workgroup a short grid leaves on a CU sit on four SIMDs.
//
// Rows a work item does not own: every global address of a workgroup is inside its own (sequence, head) -- 64 rows of q, k, v, dq, dk,
// dv at ((seq * heads + head) * 64) * D, columns below D, and dO rows seq * 64 .. seq * 64 + 63, columns head * d .. head * d + d - 1.
// There is no tail case: the grid is exactly nseq * heads workgroups, and the operand buffers need no slack behind the last sequence.
// The summation order is fixed by (D, DQK, DV), i.e. by d alone: a sequence's bits do not depend on the launch it is part of.  No
// atomics, no allocation, no synchronisation with the host.
//
// Two forms of the final store (template parameter PACKED, see the kernel): dq, dk, dv as three buffers in the layout of q, k, v, or all
// three straight into the rows of the packed dqkv [rows][3*heads*d] the weight-gradient GEMMs read (launch_attention_seq64_bwd_packed).
#include "common.h"
#include "dfot_hip.h"
#include "kernels.h"

namespace dfot {
namespace {

// the padded tile of attention_bwd.hip (its BwdCfg / tr_frag are local to that file)
template <int D>
struct Seq64BwdCfg {
  static constexpr int ROWB = D * 2 + 16;  // padded LDS row (bytes)
  static constexpr int TILE = 64 * ROWB;
  static constexpr int LDS = 4 * TILE + 3 * 64 * (int)sizeof(float);  // Q | K | V | dO | -max | 1/sum | delta
};

// A fragment of X^T for the features c0..c0+31 and the 16 tile rows of step (t2, s), in the order of the B fragment built from an
// accumulator (tile row = t2*32 + 16s + 8(j>>2) + 4h + (j&3))
template <int D>
__device__ __forceinline__ bf16x8 seq64_tr_frag(const char* tile, int c0, int t2, int s, int lane) {
  using C = Seq64BwdCfg<D>;
  const int lh = lane >> 5;
  const int rb = t2 * 32 + 16 * s + 4 * lh;
  const int q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int col = c0 + 16 * ((lane >> 4) & 1) + 4 * p4;
  const char* a0 = tile + (rb + q4) * C::ROWB + col * 2;
  const char* a1 = tile + (rb + 8 + q4) * C::ROWB + col * 2;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a1));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// the row fragment (A or B operand) of tile row `row`, contraction step ks
template <int D>
__device__ __forceinline__ bf16x8 seq64_row_frag(const char* tile, int row, int ks, int lh) {
  return *reinterpret_cast<const bf16x8*>(tile + row * Seq64BwdCfg<D>::ROWB + (ks * 2 + lh) * 16);
}

// acc[dvt][4g + j] = X^T[dvt*32 + 8g + 4lh + j][row of this lane]: scale, round and store the live columns of the lane's row.  As the
// forward's store: for every pair of groups (g = 2a, 2a+1) the two lanes of a row swap one 4-column half, after which lane lh owns the 8
// consecutive columns dvt*32 + 16a + 8lh .. +7: one 16-byte store, and only where those columns are live
template <int DV>
__device__ __forceinline__ void seq64_store_row(const f32x16 (&acc)[DV / 32], float scale, bf16* row, int lh, int d) {
#pragma unroll
  for (int dvt = 0; dvt < DV / 32; ++dvt)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      bf16x4 keep, give;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16 lo = f2bf(acc[dvt][8 * a + j] * scale), hi = f2bf(acc[dvt][8 * a + 4 + j] * scale);
        keep[j] = lh ? hi : lo;
        give[j] = lh ? lo : hi;
      }
      u32x2 w = __builtin_bit_cast(u32x2, give);
      w[0] = (unsigned)__shfl_xor((int)w[0], 32);
      w[1] = (unsigned)__shfl_xor((int)w[1], 32);
      const bf16x4 got = __builtin_bit_cast(bf16x4, w);
      const bf16x4 c0 = lh ? got : keep, c1 = lh ? keep : got;  // columns +0..3, +4..7
      const int c = dvt * 32 + 16 * a + 8 * lh;
      if (c < d) *reinterpret_cast<bf16x8*>(row + c) = bf16x8{c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    }
}

// D: row stride of q / k / v (64 or 128); DQK: head-dim columns contracted in S and dP (multiple of 16 covering d); DV: head-dim columns
// that are outputs of dQ, dK, dV (multiple of 32 covering d, >= DQK) -- the pad columns d..DV of q, k, v hold zeros; d: live columns
// PACKED: the second form of the store.  The products, their order and the roundings are those of the first form; only the address of a
// lane's row changes: row seq*64 + r of ONE buffer dQ [nseq*64][ldg] (dK, dV unused), dq at column head*d, dk at heads*d + head*d, dv at
// 2*heads*d + head*d -- the layout qkv_grad_pack_kernel (no RoPE) copies the first form's three buffers into, so that copy and its
// launch drop out of a spatial block's backward.  Still 16-byte stores of live columns only: with d % 8 == 0 and ldg % 8 == 0 every one
// is aligned, inside the workgroup's own 64 rows and below column 3*heads*d <= ldg.
template <int D, int DQK, int DV, bool PACKED>
__global__ __launch_bounds__(256) void attn_seq64_bwd_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                             const bf16* __restrict__ V, const bf16* __restrict__ dO, long ldo,
                                                             bf16* __restrict__ dQ, bf16* __restrict__ dK, bf16* __restrict__ dV, long ldg,
                                                             int heads, int d, float sq, float sk_scale) {
  static_assert(DQK % 16 == 0 && DV % 32 == 0 && DQK <= DV && DV <= D, "head-dim sub-range");
  using C = Seq64BwdCfg<D>;
  constexpr int CH = DV / 8;          // staged 16-byte chunks per row
  constexpr int PT = 64 * CH / 256;   // chunks per thread and tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sq_ = smem;
  char* sk = smem + C::TILE;
  char* sv = smem + 2 * C::TILE;
  char* so = smem + 3 * C::TILE;
  float* snmx = reinterpret_cast<float*>(smem + 4 * C::TILE);  // -max[q]
  float* sinv = snmx + 64;                                     // 1 / sum[q]
  float* sdl = sinv + 64;                                      // delta[q]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 31, lh = lane >> 5;
  const int bh = blockIdx.x;  // (sequence, head)
  const long base = (long)bh * 64 * D;
  const bf16* Ob = dO + (long)(bh / heads) * 64 * ldo + (long)(bh % heads) * d;

  // global -> registers (all loads in flight together) -> LDS
  bf16x8 rq[PT], rk[PT], rv[PT], ro[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int e = tid + 256 * i, row = e / CH, col = (e % CH) * 8;
    rq[i] = *reinterpret_cast<const bf16x8*>(Q + base + row * D + col);
    rk[i] = *reinterpret_cast<const bf16x8*>(K + base + row * D + col);
    rv[i] = *reinterpret_cast<const bf16x8*>(V + base + row * D + col);
    const bf16 z = f2bf(0.f);
    ro[i] = col < d ? *reinterpret_cast<const bf16x8*>(Ob + (long)row * ldo + col) : bf16x8{z, z, z, z, z, z, z, z};
  }
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int e = tid + 256 * i, off = (e / CH) * C::ROWB + (e % CH) * 16;
    *reinterpret_cast<bf16x8*>(sq_ + off) = rq[i];
    *reinterpret_cast<bf16x8*>(sk + off) = rk[i];
    *reinterpret_cast<bf16x8*>(sv + off) = rv[i];
    *reinterpret_cast<bf16x8*>(so + off) = ro[i];
  }
  __syncthreads();

  // ---- S and dP of this wave's 32 own rows (lane lq) against all 64 rows of the other side: own rows are the B operand, the other
  // side's rows the A operand, so the two roles run the same products on swapped tiles.  Register 4g + j of tile t2 is the other side's
  // row t2*32 + 8g + 4lh + j ----
  const bool qrole = wave < 2;  // wave-uniform
  const int own0 = (wave & 1) * 32;
  // this lane's output row of dq / dk / dv
  const long cdim = (long)heads * d;
  const long orow = PACKED ? ((long)(bh / heads) * 64 + own0 + lq) * ldg + (long)(bh % heads) * d : base + (long)(own0 + lq) * D;
  bf16* const dq_row = dQ + orow;
  bf16* const dk_row = PACKED ? dQ + orow + cdim : dK + orow;
  bf16* const dv_row = PACKED ? dQ + orow + 2 * cdim : dV + orow;
  const char* s_own = qrole ? sq_ : sk;
  const char* p_own = qrole ? so : sv;
  const char* s_oth = qrole ? sk : sq_;
  const char* p_oth = qrole ? sv : so;
  f32x16 sacc[2], pacc[2];
  {
    bf16x8 sf[DQK / 16], pf[DQK / 16];
#pragma unroll
    for (int ks = 0; ks < DQK / 16; ++ks) {
      sf[ks] = seq64_row_frag<D>(s_own, own0 + lq, ks, lh);
      pf[ks] = seq64_row_frag<D>(p_own, own0 + lq, ks, lh);
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[t2][r] = 0.f, pacc[t2][r] = 0.f;
      const int row = t2 * 32 + lq;
#pragma unroll
      for (int ks = 0; ks < DQK / 16; ++ks) {
        sacc[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(seq64_row_frag<D>(s_oth, row, ks, lh), sf[ks], sacc[t2], 0, 0, 0);
        pacc[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(seq64_row_frag<D>(p_oth, row, ks, lh), pf[ks], pacc[t2], 0, 0, 0);
      }
    }
  }
  bf16x8 dsf[2][2];
  if (qrole) {
    // single-pass softmax over the 64 keys of query own0 + lq (exp2 domain, fp32), then delta and dS^T
    float mx = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sacc[0][r]), sacc[1][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float rs = 0.f;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sacc[t2][r] = __builtin_amdgcn_exp2f(sacc[t2][r] - mx);
        rs += sacc[t2][r];
      }
    const float inv = 1.0f / (rs + __shfl_xor(rs, 32));
    float dl = 0.f;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sacc[t2][r] *= inv;  // P
        dl = fmaf(sacc[t2][r], pacc[t2][r], dl);
      }
    dl += __shfl_xor(dl, 32);
    if (lh == 0) {
      snmx[own0 + lq] = -mx;
      sinv[own0 + lq] = inv;
      sdl[own0 + lq] = dl;
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) dsf[t2][s][j] = f2bf(sacc[t2][8 * s + j] * (pacc[t2][8 * s + j] - dl));
  }
  __syncthreads();  // the statistics of all 64 queries are in LDS
  if (qrole) {
    // dQ^T[c][q] = K^T[c][key] dS^T[key][q]
    f32x16 acc[DV / 32];
#pragma unroll
    for (int dvt = 0; dvt < DV / 32; ++dvt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[dvt][r] = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          acc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(seq64_tr_frag<D>(sk, dvt * 32, t2, s, lane), dsf[t2][s], acc[dvt], 0, 0, 0);
    }
    seq64_store_row<DV>(acc, sq, dq_row, lh, d);
  } else {
    // P and dS of key own0 + lq from the statistics of the registers' query rows: four rows per 16-byte read
    bf16x8 pf[2][2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r0 = t2 * 32 + 8 * g + 4 * lh;
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(snmx + r0);
        const f32x4 i4 = *reinterpret_cast<const f32x4*>(sinv + r0);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(sdl + r0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = __builtin_amdgcn_exp2f(sacc[t2][4 * g + j] + m4[j]) * i4[j];
          pf[t2][g >> 1][4 * (g & 1) + j] = f2bf(p);
          dsf[t2][g >> 1][4 * (g & 1) + j] = f2bf(p * (pacc[t2][4 * g + j] - d4[j]));
        }
      }
    // dV^T[c][key] = dO^T[c][q] P[q][key],  dK^T[c][key] = Q^T[c][q] dS[q][key]
    f32x16 dva[DV / 32], dka[DV / 32];
#pragma unroll
    for (int dvt = 0; dvt < DV / 32; ++dvt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) dva[dvt][r] = 0.f, dka[dvt][r] = 0.f;
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          dva[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(seq64_tr_frag<D>(so, dvt * 32, t2, s, lane), pf[t2][s], dva[dvt], 0, 0, 0);
          dka[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(seq64_tr_frag<D>(sq_, dvt * 32, t2, s, lane), dsf[t2][s], dka[dvt], 0, 0, 0);
        }
    }
    seq64_store_row<DV>(dva, 1.0f, dv_row, lh, d);
    seq64_store_row<DV>(dka, sk_scale, dk_row, lh, d);
  }
}

template <int D, int DQK, int DV, bool PACKED>
int launch_seq64_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dq, bf16* dk, bf16* dv, long ldg, int nseq,
                     int heads, int d, hipStream_t s) {
  constexpr int lds = Seq64BwdCfg<D>::LDS;  // 35.6 KB at D = 64, 68.8 KB at D = 128: four / two workgroups per CU
  if (int rc = ensure_dyn_lds<attn_seq64_bwd_kernel<D, DQK, DV, PACKED>>(lds)) return rc;
  const float sq = 1.0f / sqrtf((float)d), sk = 0.6931471805599453f;  // as launch_attention_bwd
  hipLaunchKernelGGL((attn_seq64_bwd_kernel<D, DQK, DV, PACKED>), dim3(nseq * heads), dim3(256), lds, s, q, k, v, d_o, ldo, dq, dk, dv, ldg, heads,
                     d, sq, sk);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

// the instantiation of a head dim: (D, DQK, DV) depend on d alone, in both forms
template <bool PACKED>
int dispatch_seq64_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dq, bf16* dk, bf16* dv, long ldg, int nseq,
                       int heads, int d, hipStream_t s) {
  if (d <= 32) return launch_seq64_bwd<64, 32, 32, PACKED>(q, k, v, d_o, ldo, dq, dk, dv, ldg, nseq, heads, d, s);
  if (d <= 64) return launch_seq64_bwd<64, 64, 64, PACKED>(q, k, v, d_o, ldo, dq, dk, dv, ldg, nseq, heads, d, s);
  if (d <= 80) return launch_seq64_bwd<128, 80, 96, PACKED>(q, k, v, d_o, ldo, dq, dk, dv, ldg, nseq, heads, d, s);
  if (d <= 96) return launch_seq64_bwd<128, 96, 96, PACKED>(q, k, v, d_o, ldo, dq, dk, dv, ldg, nseq, heads, d, s);
  return launch_seq64_bwd<128, 128, 128, PACKED>(q, k, v, d_o, ldo, dq, dk, dv, ldg, nseq, heads, d, s);
}

}  // namespace

// q, k, v, dq, dk, dv [nseq][heads][64][attention_dstride(d)] as launch_attention_seq64 takes q, k, v; d_o compact as that launcher's o
int launch_attention_seq64_bwd(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dq, bf16* dk, bf16* dv, int nseq,
                               int heads, int d, hipStream_t s) {
  DFOT_REQUIRE(q && k && v && d_o && dq && dk && dv, DFOT_ERR_ARG, "attention_seq64_bwd: null pointer");
  DFOT_REQUIRE(d > 0 && d <= 128 && d % 8 == 0, DFOT_ERR_SHAPE, "attention_seq64_bwd: head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(nseq > 0 && heads > 0 && (long)nseq * heads <= 0x7fffffffL, DFOT_ERR_SHAPE, "attention_seq64_bwd: %d sequences, %d heads", nseq,
               heads);
  DFOT_REQUIRE(ldo >= (long)heads * d && ldo % 8 == 0, DFOT_ERR_SHAPE,
               "attention_seq64_bwd: d_o row stride %ld must cover %d columns and be a multiple of 8 (16-byte loads)", ldo, heads * d);
  return dispatch_seq64_bwd<false>(q, k, v, d_o, ldo, dq, dk, dv, 0, nseq, heads, d, s);
}

// q, k, v, d_o as above; dqkv [nseq*64][ldg]: row seq*64 + r holds dq | dk | dv of that token, head-major, in its first 3*heads*d columns
// (what launch_qkv_grad_pack without a rope table makes of the three buffers above); columns beyond them are not written
int launch_attention_seq64_bwd_packed(const bf16* q, const bf16* k, const bf16* v, const bf16* d_o, long ldo, bf16* dqkv, long ldg, int nseq,
                                      int heads, int d, hipStream_t s) {
  DFOT_REQUIRE(q && k && v && d_o && dqkv, DFOT_ERR_ARG, "attention_seq64_bwd_packed: null pointer");
  DFOT_REQUIRE(d > 0 && d <= 128 && d % 8 == 0, DFOT_ERR_SHAPE, "attention_seq64_bwd_packed: head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(nseq > 0 && heads > 0 && (long)nseq * heads <= 0x7fffffffL, DFOT_ERR_SHAPE, "attention_seq64_bwd_packed: %d sequences, %d heads",
               nseq, heads);
  DFOT_REQUIRE(ldo >= (long)heads * d && ldo % 8 == 0, DFOT_ERR_SHAPE,
               "attention_seq64_bwd_packed: d_o row stride %ld must cover %d columns and be a multiple of 8 (16-byte loads)", ldo, heads * d);
  DFOT_REQUIRE(ldg >= 3L * heads * d && ldg % 8 == 0, DFOT_ERR_SHAPE,
               "attention_seq64_bwd_packed: dqkv row stride %ld must cover 3 x %d columns and be a multiple of 8 (16-byte stores)", ldg, heads * d);
  return dispatch_seq64_bwd<true>(q, k, v, d_o, ldo, dqkv, nullptr, nullptr, ldg, nseq, heads, d, s);
}

}  // namespace dfot

extern "C" int dfot_op_attention_seq64_bwd(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dq, void* dk, void* dv,
                                           int nseq, int heads, int d, void* stream) {
  using namespace dfot;
  return launch_attention_seq64_bwd((const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, ldo, (bf16*)dq, (bf16*)dk, (bf16*)dv, nseq,
                                    heads, d, (hipStream_t)stream);
}

extern "C" int dfot_op_attention_seq64_bwd_packed(const void* q, const void* k, const void* v, const void* d_o, int ldo, void* dqkv, int ldg,
                                                  int nseq, int heads, int d, void* stream) {
  using namespace dfot;
  return launch_attention_seq64_bwd_packed((const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)d_o, ldo, (bf16*)dqkv, ldg, nseq, heads, d,
                                           (hipStream_t)stream);
}
