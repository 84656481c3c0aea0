// MatrixAttention core with the temporal RoPE-1D of the FacMatDiT backbone (dit_blocks.py:289-342 with multi_token = False, rope given,
// flatten_rope = False; dit_base.py:297-306): every frame is ONE token whose q / k / v are (hn x hd) matrices.
//   z [B*L*E][3h] bf16 holds (q|k|v): rows (frame l, col head c, n), columns (row head r, d);   o [B*L*E][h] in the same order.
//   One problem per (video, c, r):  S[l][l'] = scale * sum_{n,d} rope(q)[l][n][d] * rope(k)[l'][n][d],  P = softmax_l'(S),  o = P v.
//   rope: per row n, on the last axis d, position = frame index l; interleaved pairs (x[2i], x[2i+1]) -> (x[2i] c - x[2i+1] s,
//   x[2i+1] c + x[2i] s) with (c, s) = rope_cs[l][i] (table [rows >= L][hd/2][2] fp32; nullptr = no rotation).
//
// Form: one workgroup of 8 waves per problem, every q, k and v entry is read from global memory exactly once, for every 1 <= L <= 32.
//   1. S is a GEMM with M = N = L (padded to TL = 16 or 32) and reduction length R = hn*hd (4608 at XL-64-1, 4096 at S-64-1).  The order
//      of the reduction index is free as long as q and k agree on it, so the v_mfma_f32_16x16x32_bf16 operands come STRAIGHT from
//      global memory: lane (row = lane & 15, group g = lane >> 4) of reduction step s loads the 8 consecutive elements s*32 + 8g .. + 7
//      of token row l = 16*mi + row -- one 16-byte load for q (A operand) and one for k (B operand: the same lane layout with l' = row) --
//      rotates them in fp32 with the table row of l (shared by q and k), rounds to bf16 and issues NT*NT MFMAs (NT = TL/16).
//      Rows l >= L and steps past R are zero fragments that are never loaded.  The steps are split into one contiguous range per wave
//      (a wave walks along the hd-contiguous runs of z), the 8 partial TL x TL tiles are summed through LDS in wave order (no atomics:
//      the same bits every run and for every batch size).
//   2. softmax over l' in fp32 by L threads; P is kept transposed and zero-padded in LDS.
//   3. o = P v on the VALU (reduction length L <= 32): one thread per 4 consecutive d, v read once (8-byte loads), P read as LDS broadcasts.
// Arithmetic per problem at XL-64-1, L = 16: 3 * 16 * 4608 * 2 B = 442 KB read + 147 KB written for 2 * 2 * 16*16*4608 = 4.7 Mflop
// (8 flop/byte): bound by memory; the MFMA form is chosen because it needs no L x L per-thread register tile (the read-once VALU form
// of matrix_attn_kernel<LT> holds LT*LT accumulators per thread and does not scale past LT = 10), not for its rate.
#include "common.h"
#include "kernels.h"

namespace dfot {
namespace {

constexpr int MA_WAVES = 8, MA_THREADS = MA_WAVES * 64;

// NT: 16-row tiles of the token axis (TL = 16 * NT >= L); CH: bf16 elements per global access of the score phase (8 when hd % 8 == 0, else 4)
template <int NT, int CH, bool ROPE>
__global__ __launch_bounds__(MA_THREADS) void matrix_attn_rope_kernel(const bf16* __restrict__ z, bf16* __restrict__ o,
                                                                      const float* __restrict__ rope_cs, int L, int E, int h, int cc, int rr,
                                                                      float scale) {
  constexpr int TL = 16 * NT;
  constexpr int U = 4 / NT;  // reduction steps whose loads are issued together
  __shared__ __attribute__((aligned(16))) float part[MA_WAVES][TL * TL];
  __shared__ __attribute__((aligned(16))) float pt[TL * TL];  // P transposed: pt[l'][l], zero for l >= L
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / (cc * rr), c = (blockIdx.x / rr) % cc, r = blockIdx.x % rr;
  const int hn = E / cc, hd = h / rr, R = hn * hd;
  const long ldz = 3L * h;
  const bf16* zb = z + (((long)b * L) * E + c * hn) * ldz + r * hd;  // q of (frame 0, n 0); frame stride E*ldz, n stride ldz
  const long lstride = (long)E * ldz;

  for (int i = threadIdx.x; i < TL * TL; i += MA_THREADS) pt[i] = 0.f;

  // ---- 1. partial scores of this wave's range of reduction steps ----
  f32x4 acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fg = lane >> 4;
  const int steps = (R + 31) / 32, per_wave = (steps + MA_WAVES - 1) / MA_WAVES;
  const int s_end = min(steps, (wave + 1) * per_wave);
  for (int s0 = wave * per_wave; s0 < s_end; s0 += U) {
    bf16x8 qf[U][NT], kf[U][NT];
    f32x4 cs[U][NT][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // the lane's 8 reduction elements of step s0 + u: CH = 8: base .. base + 7; CH = 4: base .. + 3 and base + 16 .. + 19
      const int base0 = (s0 + u) * 32 + fg * CH, base1 = base0 + (CH == 8 ? 4 : 16);
      const bool ok0 = s0 + u < s_end && base0 < R, ok1 = s0 + u < s_end && base1 < R;
      const int n0 = base0 / hd, d0 = base0 - n0 * hd;
      const int n1 = CH == 8 ? n0 : base1 / hd, d1 = CH == 8 ? d0 + 4 : base1 - n1 * hd;
#pragma unroll
      for (int mi = 0; mi < NT; ++mi) {
        const int l = mi * 16 + frow;
        bf16x8 q8, k8;
#pragma unroll
        for (int e = 0; e < 8; ++e) q8[e] = k8[e] = (bf16)0.f;
        cs[u][mi][0] = cs[u][mi][1] = f32x4{1.f, 0.f, 1.f, 0.f};
        if (l < L) {
          const bf16* p0 = zb + l * lstride + n0 * ldz + d0;
          if constexpr (CH == 8) {
            if (ok0) {
              q8 = *reinterpret_cast<const bf16x8*>(p0);
              k8 = *reinterpret_cast<const bf16x8*>(p0 + h);
            }
          } else {
            const bf16* p1 = zb + l * lstride + n1 * ldz + d1;
            bf16x4 qa = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f}, qb = qa, ka = qa, kb = qa;
            if (ok0) {
              qa = *reinterpret_cast<const bf16x4*>(p0);
              ka = *reinterpret_cast<const bf16x4*>(p0 + h);
            }
            if (ok1) {
              qb = *reinterpret_cast<const bf16x4*>(p1);
              kb = *reinterpret_cast<const bf16x4*>(p1 + h);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              q8[e] = qa[e]; q8[4 + e] = qb[e];
              k8[e] = ka[e]; k8[4 + e] = kb[e];
            }
          }
          if constexpr (ROPE) {  // (cos, sin) of the two pairs of each 4-element half; d0, d1 are multiples of 4: 16-byte aligned
            const float* row = rope_cs + (long)l * hd;
            if (ok0) cs[u][mi][0] = *reinterpret_cast<const f32x4*>(row + d0);
            if (ok1) cs[u][mi][1] = *reinterpret_cast<const f32x4*>(row + d1);
          }
        }
        qf[u][mi] = q8;
        kf[u][mi] = k8;
      }
    }
    if constexpr (ROPE) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int mi = 0; mi < NT; ++mi)
#pragma unroll
          for (int p = 0; p < 4; ++p) {  // pair p: elements 2p, 2p + 1
            const float co = cs[u][mi][p >> 1][(p & 1) * 2], si = cs[u][mi][p >> 1][(p & 1) * 2 + 1];
            const float qa = bf2f(qf[u][mi][2 * p]), qb = bf2f(qf[u][mi][2 * p + 1]);
            const float ka = bf2f(kf[u][mi][2 * p]), kb = bf2f(kf[u][mi][2 * p + 1]);
            qf[u][mi][2 * p] = f2bf(qa * co - qb * si);
            qf[u][mi][2 * p + 1] = f2bf(qb * co + qa * si);
            kf[u][mi][2 * p] = f2bf(ka * co - kb * si);
            kf[u][mi][2 * p + 1] = f2bf(kb * co + ka * si);
          }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int mi = 0; mi < NT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[u][mi], kf[u][ni], acc[mi][ni], 0, 0, 0);
  }
  // C layout of the 16x16 MFMA: register i of lane = (row (lane >> 4) * 4 + i, col lane & 15)
#pragma unroll
  for (int mi = 0; mi < NT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[wave][(mi * 16 + fg * 4 + i) * TL + ni * 16 + frow] = acc[mi][ni][i];
  __syncthreads();
  for (int i = threadIdx.x; i < TL * TL; i += MA_THREADS) {
    float t = part[0][i];
#pragma unroll
    for (int w = 1; w < MA_WAVES; ++w) t += part[w][i];
    part[0][i] = t * scale;  // entry i is read and written by this thread only
  }
  __syncthreads();

  // ---- 2. softmax over l' ----
  if (threadIdx.x < L) {
    const float* row = part[0] + threadIdx.x * TL;
    float mx = row[0];
    for (int j = 1; j < L; ++j) mx = fmaxf(mx, row[j]);
    float sum = 0.f;
    for (int j = 0; j < L; ++j) sum += __expf(row[j] - mx);
    const float inv = 1.0f / sum;
    for (int j = 0; j < L; ++j) pt[j * TL + threadIdx.x] = __expf(row[j] - mx) * inv;
  }
  __syncthreads();

  // ---- 3. o = P v: one thread per (n, 4 consecutive d) ----
  const bf16* vb = zb + 2 * h;
  bf16* ob = o + (((long)b * L) * E + c * hn) * h + r * hd;
  const long ostride = (long)E * h;
  for (int e = threadIdx.x; e < R / 4; e += MA_THREADS) {
    const int n = (e * 4) / hd, d = e * 4 - n * hd;
    float a[TL][4];
#pragma unroll
    for (int l = 0; l < TL; ++l)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[l][j] = 0.f;
    for (int l2 = 0; l2 < L; ++l2) {
      const bf16x4 v4 = *reinterpret_cast<const bf16x4*>(vb + l2 * lstride + n * ldz + d);
      const float vf[4] = {bf2f(v4[0]), bf2f(v4[1]), bf2f(v4[2]), bf2f(v4[3])};
#pragma unroll
      for (int l = 0; l < TL; l += 4) {
        const f32x4 p4 = *reinterpret_cast<const f32x4*>(pt + l2 * TL + l);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) a[l + i][j] = fmaf(p4[i], vf[j], a[l + i][j]);
      }
    }
#pragma unroll
    for (int l = 0; l < TL; ++l)
      if (l < L) {
        bf16x4 o4;
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = f2bf(a[l][j]);
        *reinterpret_cast<bf16x4*>(ob + l * ostride + (long)n * h + d) = o4;
      }
  }
}

}  // namespace

int launch_matrix_attn_rope(const bf16* z, bf16* o, const float* rope_cs, int batch, int L, int E, int h, int cc, int rr, float scale,
                            hipStream_t s) {
  DFOT_REQUIRE(z && o, DFOT_ERR_ARG, "matrix attention: null pointer");
  DFOT_REQUIRE(L >= 1 && L <= 32, DFOT_ERR_SHAPE, "matrix attention: %d frame tokens (1 to 32 are supported)", L);
  DFOT_REQUIRE(batch > 0 && E > 0 && h > 0 && cc > 0 && rr > 0, DFOT_ERR_SHAPE, "matrix attention: batch %d, E %d, h %d, heads (%d, %d)", batch, E, h,
               cc, rr);
  DFOT_REQUIRE(E % cc == 0, DFOT_ERR_SHAPE, "matrix attention: embed_col_dim %d is not divisible by %d col heads", E, cc);
  DFOT_REQUIRE(h % rr == 0, DFOT_ERR_SHAPE, "matrix attention: embed_row_dim %d is not divisible by %d row heads", h, rr);
  const int hd = h / rr;
  DFOT_REQUIRE(hd % 4 == 0, DFOT_ERR_SHAPE, "matrix attention: row head dim %d must be a multiple of 4", hd);
  DFOT_REQUIRE((long)batch * cc * rr <= 0x7fffffffL && (long)(E / cc) * hd <= (1L << 26), DFOT_ERR_SHAPE,
               "matrix attention: %ld problems of %ld entries", (long)batch * cc * rr, (long)(E / cc) * hd);
  const dim3 grid(batch * cc * rr), blk(MA_THREADS);
#define LAUNCH(NT, CH, ROPE) hipLaunchKernelGGL((matrix_attn_rope_kernel<NT, CH, ROPE>), grid, blk, 0, s, z, o, rope_cs, L, E, h, cc, rr, scale)
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

extern "C" int dfot_op_matrix_attention_rope(const void* z, void* o, const float* rope_cs, int batch, int L, int E, int h, int cc, int rr,
                                             float scale, void* stream) {
  using namespace dfot;
  return launch_matrix_attn_rope((const bf16*)z, (bf16*)o, rope_cs, batch, L, E, h, cc, rr, scale, (hipStream_t)stream);
}
