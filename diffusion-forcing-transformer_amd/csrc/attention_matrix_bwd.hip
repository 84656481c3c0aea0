// Backward of matrix_attn_rope_kernel (attention_matrix.hip): the MatrixAttention core of the FacMatDiT backbone with its temporal RoPE-1D.
//   z [B*L*E][3h] bf16 (q|k|v), d_o [B*L*E][h] bf16 (the forward's layouts), rope_cs [rows >= L][hd/2][2] fp32 or nullptr
//   -> dz [B*L*E][3h] bf16 (dq|dk|dv).  One problem per (video, col head c, row head r), R = hn*hd entries per token:
//     q~ = rope(q), k~ = rope(k)                 (fp32 rotation rounded to bf16 exactly as the forward does: S is the forward's S)
//     S  = scale q~ k~^T,  dP = d_o v^T          (L x L, reduction length R)
//     P  = softmax_l'(S),  dS = P o (dP - sum_l' P o dP) scale
//     dq~ = dS k~,  dk~ = dS^T q~,  dv = P^T d_o
//     dq = rope^-1(dq~), dk = rope^-1(dk~)       (the transposed rotation, angle of the gradient's own token row)
//
// Form: one workgroup of 8 waves per problem, as the forward.
//   1. The two Gram matrices are the forward's phase 1 run twice: v_mfma_f32_16x16x32_bf16 operands straight from global memory in the
//      MFMA's lane layout, one contiguous range of reduction steps per wave, the 8 partial TL x TL tiles summed through LDS in wave
//      order (no atomics).  S is reduced first and the partial buffer reused for dP (two sets would be 64 KB at TL = 32).
//   2. softmax and dS in fp32 by L threads; P and dS stay in LDS, dS in both orientations (phase 3 reads rows of them as broadcasts).
//   3. VALU, one thread per (n, 4 consecutive d), three passes of TL x 4 fp32 accumulators: dq reads k, dk reads q, dv reads d_o
//      (8-byte loads, mostly L2 hits of phase 1).  Both elements of a RoPE pair lie inside a thread's four d: the rotation of the
//      operand (kept in fp32) and the inverse rotation of the result are thread-local.
// Fixed summation order everywhere: a video gives the same bits alone, in a batch and on repeat.  Traffic per problem: (4 reads +
// 3 writes) L R 2 B from HBM, phase 3's re-reads from L2 / MALL.
#include "common.h"
#include "kernels.h"

namespace dfot {
namespace {

constexpr int MB_WAVES = 8, MB_THREADS = MB_WAVES * 64;

// partial Gram tile of this wave's reduction steps: out[l][l'] = sum_e A[l][e] B[l'][e], e = (n, d) over R = hn*hd entries;
// a / b point at (frame 0, n 0, d 0) of the head, frame strides la / lb, n strides na / nb.  ROPE rotates both operands with the table
// row of their own token (fp32, rounded to bf16).  The wave's tile is stored to `part` (TL*TL floats).
template <int NT, int CH, bool ROPE>
__device__ __forceinline__ void gram_partial(const bf16* __restrict__ a, long la, long na, const bf16* __restrict__ b, long lb, long nb,
                                             const float* __restrict__ rope_cs, int L, int hd, int R, int wave, int lane,
                                             float* __restrict__ part) {
  constexpr int TL = 16 * NT;
  constexpr int U = 4 / NT;  // reduction steps whose loads are issued together
  f32x4 acc[NT][NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fg = lane >> 4;
  const int steps = (R + 31) / 32, per_wave = (steps + MB_WAVES - 1) / MB_WAVES;
  const int s_end = min(steps, (wave + 1) * per_wave);
  for (int s0 = wave * per_wave; s0 < s_end; s0 += U) {
    bf16x8 af[U][NT], bfr[U][NT];
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
        bf16x8 a8, b8;
#pragma unroll
        for (int e = 0; e < 8; ++e) a8[e] = b8[e] = (bf16)0.f;
        cs[u][mi][0] = cs[u][mi][1] = f32x4{1.f, 0.f, 1.f, 0.f};
        if (l < L) {
          if constexpr (CH == 8) {
            if (ok0) {
              a8 = *reinterpret_cast<const bf16x8*>(a + l * la + n0 * na + d0);
              b8 = *reinterpret_cast<const bf16x8*>(b + l * lb + n0 * nb + d0);
            }
          } else {
            bf16x4 aa = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f}, ab = aa, ba = aa, bb = aa;
            if (ok0) {
              aa = *reinterpret_cast<const bf16x4*>(a + l * la + n0 * na + d0);
              ba = *reinterpret_cast<const bf16x4*>(b + l * lb + n0 * nb + d0);
            }
            if (ok1) {
              ab = *reinterpret_cast<const bf16x4*>(a + l * la + n1 * na + d1);
              bb = *reinterpret_cast<const bf16x4*>(b + l * lb + n1 * nb + d1);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              a8[e] = aa[e]; a8[4 + e] = ab[e];
              b8[e] = ba[e]; b8[4 + e] = bb[e];
            }
          }
          if constexpr (ROPE) {  // (cos, sin) of the two pairs of each 4-element half; d0, d1 are multiples of 4: 16-byte aligned
            const float* row = rope_cs + (long)l * hd;
            if (ok0) cs[u][mi][0] = *reinterpret_cast<const f32x4*>(row + d0);
            if (ok1) cs[u][mi][1] = *reinterpret_cast<const f32x4*>(row + d1);
          }
        }
        af[u][mi] = a8;
        bfr[u][mi] = b8;
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
            const float xa = bf2f(af[u][mi][2 * p]), xb = bf2f(af[u][mi][2 * p + 1]);
            const float ya = bf2f(bfr[u][mi][2 * p]), yb = bf2f(bfr[u][mi][2 * p + 1]);
            af[u][mi][2 * p] = f2bf(xa * co - xb * si);
            af[u][mi][2 * p + 1] = f2bf(xb * co + xa * si);
            bfr[u][mi][2 * p] = f2bf(ya * co - yb * si);
            bfr[u][mi][2 * p + 1] = f2bf(yb * co + ya * si);
          }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int mi = 0; mi < NT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][mi], bfr[u][ni], acc[mi][ni], 0, 0, 0);
  }
  // C layout of the 16x16 MFMA: register i of lane = (row (lane >> 4) * 4 + i, col lane & 15)
#pragma unroll
  for (int mi = 0; mi < NT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[(mi * 16 + fg * 4 + i) * TL + ni * 16 + frow] = acc[mi][ni][i];
}

// NT: 16-row tiles of the token axis (TL = 16 * NT >= L); CH: bf16 elements per global access of phase 1 (8 when hd % 8 == 0, else 4)
template <int NT, int CH, bool ROPE>
__global__ __launch_bounds__(MB_THREADS) void matrix_attn_rope_bwd_kernel(const bf16* __restrict__ z, const bf16* __restrict__ d_o,
                                                                          const float* __restrict__ rope_cs, bf16* __restrict__ dz, int L, int E,
                                                                          int h, int cc, int rr, float scale) {
  constexpr int TL = 16 * NT;
  __shared__ __attribute__((aligned(16))) float part[MB_WAVES][TL * TL];
  __shared__ __attribute__((aligned(16))) float sp[TL * TL];   // S, then P[l][l']
  __shared__ __attribute__((aligned(16))) float sd[TL * TL];   // dP, then dS[l][l']
  __shared__ __attribute__((aligned(16))) float sdt[TL * TL];  // dS transposed: sdt[l'][l]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / (cc * rr), c = (blockIdx.x / rr) % cc, r = blockIdx.x % rr;
  const int hn = E / cc, hd = h / rr, R = hn * hd;
  const long ldz = 3L * h;
  const long zoff = (((long)b * L) * E + c * hn) * ldz + r * hd;  // q of (frame 0, n 0); frame stride E*ldz, n stride ldz
  const bf16* zb = z + zoff;
  const bf16* gb = d_o + (((long)b * L) * E + c * hn) * h + r * hd;
  const long lstride = (long)E * ldz, gstride = (long)E * h;

  // ---- 1. S = q~ k~^T, then dP = d_o v^T: per-wave partial tiles summed in wave order ----
  gram_partial<NT, CH, ROPE>(zb, lstride, ldz, zb + h, lstride, ldz, rope_cs, L, hd, R, wave, lane, part[wave]);
  __syncthreads();
  for (int i = threadIdx.x; i < TL * TL; i += MB_THREADS) {
    float t = part[0][i];
#pragma unroll
    for (int w = 1; w < MB_WAVES; ++w) t += part[w][i];
    sp[i] = t * scale;
  }
  __syncthreads();
  gram_partial<NT, CH, false>(gb, gstride, h, zb + 2 * h, lstride, ldz, nullptr, L, hd, R, wave, lane, part[wave]);
  __syncthreads();
  for (int i = threadIdx.x; i < TL * TL; i += MB_THREADS) {
    float t = part[0][i];
#pragma unroll
    for (int w = 1; w < MB_WAVES; ++w) t += part[w][i];
    sd[i] = t;
  }
  __syncthreads();

  // ---- 2. softmax over l' and dS; rows and columns past L are zero in all three tiles ----
  if (threadIdx.x < TL) {
    const int l = threadIdx.x;
    float* prow = sp + l * TL;
    float* drow = sd + l * TL;
    if (l < L) {
      float mx = prow[0];
      for (int j = 1; j < L; ++j) mx = fmaxf(mx, prow[j]);
      float sum = 0.f;
      for (int j = 0; j < L; ++j) sum += __expf(prow[j] - mx);
      const float inv = 1.0f / sum;
      float dot = 0.f;
      for (int j = 0; j < L; ++j) {
        const float pj = __expf(prow[j] - mx) * inv;
        prow[j] = pj;
        dot += pj * drow[j];
      }
      for (int j = 0; j < L; ++j) {
        const float ds = prow[j] * (drow[j] - dot) * scale;
        drow[j] = ds;
        sdt[j * TL + l] = ds;
      }
      for (int j = L; j < TL; ++j) prow[j] = drow[j] = sdt[j * TL + l] = 0.f;
    } else {
      for (int j = 0; j < TL; ++j) prow[j] = drow[j] = sdt[j * TL + l] = 0.f;
    }
  }
  __syncthreads();

  // ---- 3. dq = rope^-1(dS k~), dk = rope^-1(dS^T q~), dv = P^T d_o: one thread per (n, 4 consecutive d) ----
  bf16* dzb = dz + zoff;
  for (int e = threadIdx.x; e < R / 4; e += MB_THREADS) {
    const int n = (e * 4) / hd, d = e * 4 - n * hd;
    float a[TL][4];
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      // pass 0: dq (operand k~, weights dS^T rows); 1: dk (operand q~, weights dS rows); 2: dv (operand d_o, weights P rows)
      const bf16* src = pass == 0 ? zb + h : (pass == 1 ? zb : gb);
      const long ls = pass == 2 ? gstride : lstride, ns = pass == 2 ? (long)h : ldz;
      const float* wt = pass == 0 ? sdt : (pass == 1 ? sd : sp);
#pragma unroll
      for (int l = 0; l < TL; ++l)
#pragma unroll
        for (int j = 0; j < 4; ++j) a[l][j] = 0.f;
      for (int l2 = 0; l2 < L; ++l2) {
        const bf16x4 x4 = *reinterpret_cast<const bf16x4*>(src + l2 * ls + n * ns + d);
        float xf[4] = {bf2f(x4[0]), bf2f(x4[1]), bf2f(x4[2]), bf2f(x4[3])};
        if (ROPE && pass < 2) {
          const f32x4 cs = *reinterpret_cast<const f32x4*>(rope_cs + (long)l2 * hd + d);
          const float x0 = xf[0], x1 = xf[1], x2 = xf[2], x3 = xf[3];
          xf[0] = x0 * cs[0] - x1 * cs[1];
          xf[1] = x1 * cs[0] + x0 * cs[1];
          xf[2] = x2 * cs[2] - x3 * cs[3];
          xf[3] = x3 * cs[2] + x2 * cs[3];
        }
#pragma unroll
        for (int l = 0; l < TL; l += 4) {
          const f32x4 w4 = *reinterpret_cast<const f32x4*>(wt + l2 * TL + l);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[l + i][j] = fmaf(w4[i], xf[j], a[l + i][j]);
        }
      }
#pragma unroll
      for (int l = 0; l < TL; ++l)
        if (l < L) {
          float g0 = a[l][0], g1 = a[l][1], g2 = a[l][2], g3 = a[l][3];
          if (ROPE && pass < 2) {  // transposed rotation with the angle of the gradient's own row l
            const f32x4 cs = *reinterpret_cast<const f32x4*>(rope_cs + (long)l * hd + d);
            const float t0 = g0 * cs[0] + g1 * cs[1], t1 = g1 * cs[0] - g0 * cs[1];
            const float t2 = g2 * cs[2] + g3 * cs[3], t3 = g3 * cs[2] - g2 * cs[3];
            g0 = t0; g1 = t1; g2 = t2; g3 = t3;
          }
          const bf16x4 o4 = {f2bf(g0), f2bf(g1), f2bf(g2), f2bf(g3)};
          *reinterpret_cast<bf16x4*>(dzb + l * lstride + n * ldz + (pass == 0 ? 0 : (pass == 1 ? h : 2 * h)) + d) = o4;
        }
    }
  }
}

}  // namespace

int launch_matrix_attn_rope_bwd(const bf16* z, const bf16* d_o, const float* rope_cs, bf16* dz, int batch, int L, int E, int h, int cc, int rr,
                                float scale, hipStream_t s) {
  DFOT_REQUIRE(z && d_o && dz, DFOT_ERR_ARG, "matrix attention backward: null pointer");
  DFOT_REQUIRE(dz != z && dz != d_o, DFOT_ERR_ARG, "matrix attention backward: dz must not alias z or d_o");
  DFOT_REQUIRE(L >= 1 && L <= 32, DFOT_ERR_SHAPE, "matrix attention backward: %d frame tokens (1 to 32 are supported)", L);
  DFOT_REQUIRE(batch > 0 && E > 0 && h > 0 && cc > 0 && rr > 0, DFOT_ERR_SHAPE, "matrix attention backward: batch %d, E %d, h %d, heads (%d, %d)",
               batch, E, h, cc, rr);
  DFOT_REQUIRE(E % cc == 0, DFOT_ERR_SHAPE, "matrix attention backward: embed_col_dim %d is not divisible by %d col heads", E, cc);
  DFOT_REQUIRE(h % rr == 0, DFOT_ERR_SHAPE, "matrix attention backward: embed_row_dim %d is not divisible by %d row heads", h, rr);
  const int hd = h / rr;
  DFOT_REQUIRE(hd % 4 == 0, DFOT_ERR_SHAPE, "matrix attention backward: row head dim %d must be a multiple of 4", hd);
  DFOT_REQUIRE((long)batch * cc * rr <= 0x7fffffffL && (long)(E / cc) * hd <= (1L << 26), DFOT_ERR_SHAPE,
               "matrix attention backward: %ld problems of %ld entries", (long)batch * cc * rr, (long)(E / cc) * hd);
  const dim3 grid(batch * cc * rr), blk(MB_THREADS);
#define LAUNCH(NT, CH, ROPE) \
  hipLaunchKernelGGL((matrix_attn_rope_bwd_kernel<NT, CH, ROPE>), grid, blk, 0, s, z, d_o, rope_cs, dz, L, E, h, cc, rr, scale)
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

extern "C" int dfot_op_matrix_attention_rope_bwd(const void* z, const void* d_o, const float* rope_cs, void* dz, int batch, int L, int E, int h,
                                                 int cc, int rr, float scale, void* stream) {
  using namespace dfot;
  return launch_matrix_attn_rope_bwd((const bf16*)z, (const bf16*)d_o, rope_cs, (bf16*)dz, batch, L, E, h, cc, rr, scale, (hipStream_t)stream);
}
