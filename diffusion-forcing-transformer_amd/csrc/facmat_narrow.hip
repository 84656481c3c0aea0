// Left factors of the MatrixDiTBlock at narrow column widths (FacMatDiT, 1 <= embed_col_dim <= 32; gfx950).
//
//   contract: w[f][e][d] = sum_p u[e][p] * m[f][p][d]      m [frames][P][h]  ->  w [frames][E][h]     (qkv_u applied to the modulated frame)
//   expand:   s[f][p][d] = sum_e u[p][e] * o[f][e][d]      o [frames][E][h]  ->  s [frames][P][h]     (proj_u applied to the attention output)
//
// At E >= 64 these are tensor-core GEMMs between two per-frame transposes (dit.hip): the contracted index (p, resp. e) is the ROW index
// of the activation tile, so an MFMA operand would hold elements that lie h apart in memory.  At E <= 32 the products are streaming
// kernels -- contract reads P*h values per frame and writes E/P of that, expand is the mirror -- and they run on the VALU in the natural
// [row][d] layout: a lane owns 8 consecutive d columns (one 16-byte access per row), and a row of the tile times one scalar of u is 8
// FMAs with no data movement.  No transpose launch, no LDS image of the tile.
//
// Work split: one wave (= one workgroup) owns 64 d columns of one frame -- 8 lanes across d, 8 lane groups across rows.
//   contract: lane group g sums the rows [g*P/8, (g+1)*P/8) in ascending p; the 8 partial sums meet in LDS and are added in ascending g.
//   expand:   lane group g owns 4 of the 32 output rows of the workgroup's row block; every output sums e in ascending order.
// Both orders depend on (P, E) alone: a frame's bits do not depend on the launch it is part of.  No atomics.
// Every global address of a workgroup lies inside its own frame (and u); nothing is read or written outside the operands' extents
// m / s [frames*P*h], w / o [frames*E*h], u [E*P].
#include "common.h"
#include "dfot_hip.h"
#include "kernels.h"

namespace dfot {
namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// EC: columns of u (values of e) carried per pass over the frame's tile; E > EC runs ceil(E / EC) passes (the re-read hits L1 / L2:
// a workgroup's slice of the tile is P * 128 bytes)
template <int EC>
__global__ __launch_bounds__(64) void facmat_contract_kernel(const bf16* __restrict__ m, const bf16* __restrict__ u, bf16* __restrict__ w,
                                                             int P, int h, int E) {
  __shared__ __attribute__((aligned(16))) float red[8][EC][64];
  const int lane = threadIdx.x, dl = lane & 7, pg = lane >> 3;
  const int nch = h >> 6;
  const int frame = blockIdx.x / nch, ch = blockIdx.x % nch;
  const int rows = P >> 3;  // rows per lane group: a multiple of 8
  const bf16* mp = m + ((long)frame * P + (long)pg * rows) * h + ch * 64 + dl * 8;
  const bf16* up = u + pg * rows;
  for (int e0 = 0; e0 < E; e0 += EC) {
    f32x2 acc[EC][4];  // pairs of columns: one v_pk_fma_f32 per pair
#pragma unroll
    for (int j = 0; j < EC; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[j][c] = f32x2{0.f, 0.f};
    for (int p0 = 0; p0 < rows; p0 += 8) {
      bf16x8 uv[EC];
#pragma unroll
      for (int j = 0; j < EC; ++j) {
        const int e = e0 + j < E ? e0 + j : E - 1;  // columns past E: a valid address; the sums are never stored
        uv[j] = ld8(up + (long)e * P + p0);
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const bf16x8 mv = ld8(mp + (long)(p0 + r) * h);
        f32x2 mf[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) mf[c] = f32x2{bf2f(mv[2 * c]), bf2f(mv[2 * c + 1])};
#pragma unroll
        for (int j = 0; j < EC; ++j) {
          const float uf = bf2f(uv[j][r]);
          const f32x2 u2 = {uf, uf};
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[j][c] = __builtin_elementwise_fma(u2, mf[c], acc[j][c]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < EC; ++j) {
      *reinterpret_cast<f32x4*>(&red[pg][j][dl * 8]) = f32x4{acc[j][0][0], acc[j][0][1], acc[j][1][0], acc[j][1][1]};
      *reinterpret_cast<f32x4*>(&red[pg][j][dl * 8 + 4]) = f32x4{acc[j][2][0], acc[j][2][1], acc[j][3][0], acc[j][3][1]};
    }
    __syncthreads();
    if (lane < EC * 8) {  // lane -> (e0 + j, 8 columns): the 8 partial sums in ascending lane group
      const int j = lane >> 3;
      f32x4 lo = *reinterpret_cast<const f32x4*>(&red[0][j][dl * 8]), hi = *reinterpret_cast<const f32x4*>(&red[0][j][dl * 8 + 4]);
#pragma unroll
      for (int g = 1; g < 8; ++g) {
        lo += *reinterpret_cast<const f32x4*>(&red[g][j][dl * 8]);
        hi += *reinterpret_cast<const f32x4*>(&red[g][j][dl * 8 + 4]);
      }
      if (e0 + j < E) {
        bf16x8 ov;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          ov[c] = f2bf(lo[c]);
          ov[c + 4] = f2bf(hi[c]);
        }
        *reinterpret_cast<bf16x8*>(w + ((long)frame * E + e0 + j) * h + ch * 64 + dl * 8) = ov;
      }
    }
    __syncthreads();
  }
}

constexpr int XR = 4;  // output rows per lane of the expand kernel: 8 lane groups x 4 rows = 32 rows per workgroup

// VEC: E % 8 == 0, the rows of u are read with 16-byte loads; otherwise element by element (E = 1, 3, ...: a few values per row)
template <bool VEC>
__global__ __launch_bounds__(64) void facmat_expand_kernel(const bf16* __restrict__ o, const bf16* __restrict__ u, bf16* __restrict__ s, int P,
                                                           int h, int E) {
  const int lane = threadIdx.x, dl = lane & 7, rg = lane >> 3;
  const int nch = h >> 6, npb = P >> 5;
  const int ch = blockIdx.x % nch, pb = (blockIdx.x / nch) % npb, frame = blockIdx.x / (nch * npb);
  const int p_first = pb * 32 + rg * XR;  // this lane's XR output rows
  const bf16* op = o + (long)frame * E * h + ch * 64 + dl * 8;
  const bf16* up = u + (long)p_first * E;
  f32x2 acc[XR][4];  // pairs of columns: one v_pk_fma_f32 per pair
#pragma unroll
  for (int r = 0; r < XR; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = f32x2{0.f, 0.f};
  for (int e0 = 0; e0 < E; e0 += 8) {
    bf16x8 uv[XR];
    if (VEC) {
#pragma unroll
      for (int r = 0; r < XR; ++r) uv[r] = ld8(up + (long)r * E + e0);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = e0 + j;
      if (!VEC && e >= E) break;
      const bf16x8 ov = ld8(op + (long)e * h);
      f32x2 of[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) of[c] = f32x2{bf2f(ov[2 * c]), bf2f(ov[2 * c + 1])};
#pragma unroll
      for (int r = 0; r < XR; ++r) {
        const float uf = VEC ? bf2f(uv[r][j]) : bf2f(up[(long)r * E + e]);
        const f32x2 u2 = {uf, uf};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_elementwise_fma(u2, of[c], acc[r][c]);
      }
    }
  }
  bf16* sp = s + ((long)frame * P + p_first) * h + ch * 64 + dl * 8;
#pragma unroll
  for (int r = 0; r < XR; ++r) {
    bf16x8 sv;
#pragma unroll
    for (int c = 0; c < 8; ++c) sv[c] = f2bf(acc[r][c >> 1][c & 1]);
    *reinterpret_cast<bf16x8*>(sp + (long)r * h) = sv;
  }
}

// the shape contract of both launchers, checked before any device work
int facmat_narrow_check(const char* op, const void* a, const void* u, const void* out, int frames, int P, int h, int E) {
  DFOT_REQUIRE(a && u && out, DFOT_ERR_ARG, "%s: null pointer", op);
  DFOT_REQUIRE(((uintptr_t)a | (uintptr_t)u | (uintptr_t)out) % 16 == 0, DFOT_ERR_ARG, "%s: operands must be 16-byte aligned", op);
  DFOT_REQUIRE(E >= 1 && E <= 32, DFOT_ERR_SHAPE, "%s: embed_col_dim %d outside 1 .. 32 (wider factors are GEMMs)", op, E);
  DFOT_REQUIRE(P > 0 && P % 64 == 0, DFOT_ERR_SHAPE, "%s: %d patches per frame must be a positive multiple of 64", op, P);
  DFOT_REQUIRE(h > 0 && h % 64 == 0 && h <= 2048, DFOT_ERR_SHAPE, "%s: embed_row_dim %d must be a multiple of 64, <= 2048", op, h);
  DFOT_REQUIRE(frames >= 1 && (long)frames * (h / 64) * (P / 32) <= 0x7fffffffL, DFOT_ERR_SHAPE, "%s: %d frames of %d x %d", op, frames, P, h);
  return DFOT_OK;
}

}  // namespace

int launch_facmat_contract(const bf16* m, const bf16* u, bf16* w, int frames, int P, int h, int E, hipStream_t s) {
  int rc = facmat_narrow_check("facmat_contract", m, u, w, frames, P, h, E);
  if (rc) return rc;
  const dim3 grid(frames * (h / 64)), blk(64);
  if (E == 1)
    hipLaunchKernelGGL(facmat_contract_kernel<1>, grid, blk, 0, s, m, u, w, P, h, E);
  else if (E <= 4)
    hipLaunchKernelGGL(facmat_contract_kernel<4>, grid, blk, 0, s, m, u, w, P, h, E);
  else
    hipLaunchKernelGGL(facmat_contract_kernel<8>, grid, blk, 0, s, m, u, w, P, h, E);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

int launch_facmat_expand(const bf16* o, const bf16* u, bf16* sp, int frames, int P, int h, int E, hipStream_t s) {
  int rc = facmat_narrow_check("facmat_expand", o, u, sp, frames, P, h, E);
  if (rc) return rc;
  const dim3 grid(frames * (h / 64) * (P / 32)), blk(64);
  if (E % 8 == 0)
    hipLaunchKernelGGL(facmat_expand_kernel<true>, grid, blk, 0, s, o, u, sp, P, h, E);
  else
    hipLaunchKernelGGL(facmat_expand_kernel<false>, grid, blk, 0, s, o, u, sp, P, h, E);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace dfot

extern "C" int dfot_op_facmat_contract(const void* m, const void* u, void* w, int frames, int P, int h, int E, void* stream) {
  using namespace dfot;
  return launch_facmat_contract((const bf16*)m, (const bf16*)u, (bf16*)w, frames, P, h, E, (hipStream_t)stream);
}

extern "C" int dfot_op_facmat_expand(const void* o, const void* u, void* s, int frames, int P, int h, int E, void* stream) {
  using namespace dfot;
  return launch_facmat_expand((const bf16*)o, (const bf16*)u, (bf16*)s, frames, P, h, E, (hipStream_t)stream);
}
