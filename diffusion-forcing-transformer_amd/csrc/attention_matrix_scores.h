// Score phase of the FacMatDiT matrix attention as a device function, for the attention-map kernel (attention_map.hip): the q / k
// operand loads straight from z, the temporal RoPE-1D rotation, the MFMA products and the fixed-order sum of the eight waves' partial
// tiles -- statement for statement the score phase of matrix_attn_rope_kernel (attention_matrix.hip, which documents the layout of z and
// the form of the reduction).  The forward kernel keeps its own inline text: routed through this function its address arithmetic
// compiles differently, and the forward's generated code is not to change for a read-out.
#pragma once
#include "common.h"

namespace dfot {

constexpr int MA_WAVES = 8, MA_THREADS = MA_WAVES * 64;

// NT: 16-row tiles of the token axis (TL = 16 * NT >= L); CH: bf16 elements per global access (8 when hd % 8 == 0, else 4).
// zb: q of (frame 0, n 0) of the problem; frame stride lstride, n stride ldz, k at +h.  On return (after a barrier) part[0][l * TL + l']
// holds scale * <rope(q)[l], rope(k)[l']> for every l, l' < TL (zero rows / columns past L).
template <int NT, int CH, bool ROPE>
__device__ __forceinline__ void matrix_attn_scores(const bf16* zb, const float* rope_cs, int lane, int wave, int L, int h, int hd, int R,
                                                   long ldz, long lstride, float scale, float (*part)[16 * NT * 16 * NT]) {
  constexpr int TL = 16 * NT;
  constexpr int U = 4 / NT;  // reduction steps whose loads are issued together
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
}

}  // namespace dfot
