// Gradient of the two left factors U, U' of the FacMatDiT matrix block, operands as the training step leaves them (gfx950).
//
//     out[ra][rb] (fp32) = sum_f sum_d A[f][ra][d] * B[f][rb][d]        A [frames][Ra][hd], B [frames][Rb][hd] bf16, Ra, Rb in {64, 128}
//
// dU'[e][p] = sum_{f,d} o[f][e][d] ds[f][p][d] and dU[p][e] = sum_{f,d} m[f][p][d] dw1[f][e][d]: both operands already lie with the
// contracted index d contiguous, frame by frame, so this is A W^T batched over the frames and summed over the batch.  No permuted copy
// ([frames][R][hd] -> [R][frames * hd]), no operand padded to 128 rows, no memset.
//
// One workgroup = 4 waves = one 64 x 64 output tile of one slice of the frame axis; wave (i, j) owns the 32 x 32 sub-tile and one
// v_mfma_f32_32x32x16_bf16 accumulator.  A fragment of that MFMA is, per lane, 8 consecutive k of ONE row (lane & 31), the lane half
// (lane >> 5) choosing which 8 of the 16 -- exactly a 16-byte piece of a row of A or B as it lies in memory, so the fragments are loaded
// straight from global memory, no LDS.  The order of k inside the contraction is free as long as both operands agree, so the 128 k of a
// chunk are dealt out so that a lane reads one whole 128-byte line per row: lane half h, step c holds k = 64 h + 8 c .. + 8.
// The next chunk's 16 loads are issued before the 8 MFMAs of the current one.
//
// Few output tiles (1, 2 or 4) over a very long contraction (frames * hd ~ 1e5), so the frame axis is split over `slices` workgroups
// per tile; every slice stores its partial tile with plain stores to ws + slice * Ra * Rb and a second kernel sums the slices in a
// fixed order.  No atomics: the result's bits depend on the shape and the slice count alone.
// The sum is a kernel of its own here, not the trainer's slices_sum_kernel: that one walks the slices one after the other in every
// thread, which with up to 256 slices of a 64 x 64 tile is 256 dependent steps on 4 workgroups -- measured at 45 us next to 13 us for
// the products themselves.  Here 16 groups of threads take every 16th slice each and their 16 sums are added in group order.
#include "common.h"
#include "dfot_hip.h"
#include "kernels.h"

namespace dfot {
namespace {

typedef __attribute__((ext_vector_type(4))) float float4v;
constexpr int FW_KC = 128;  // k per chunk: 8 MFMA steps of 16

__global__ __launch_bounds__(256) void facmat_factor_wgrad_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B, float* __restrict__ out,
                                                                  int frames, int ra, int rb, int hd, int slices) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int slice = blockIdx.x;
  const int m0 = blockIdx.y * 64 + (wave >> 1) * 32, n0 = blockIdx.z * 64 + (wave & 1) * 32;
  // this slice's frames: the first `rem` slices take one more
  const int per = frames / slices, rem = frames % slices;
  const int f0 = slice * per + (slice < rem ? slice : rem), nf = per + (slice < rem ? 1 : 0);
  const int cpf = hd / FW_KC;   // chunks per frame
  const int nc = nf * cpf;
  // row m0 + lq of A / n0 + lq of B in frame f0, this lane half's 64 k of the chunk
  const bf16* pa = A + ((long)f0 * ra + m0 + lq) * hd + lh * 64;
  const bf16* pb = B + ((long)f0 * rb + n0 + lq) * hd + lh * 64;
  const long skip_a = (long)(ra - 1) * hd, skip_b = (long)(rb - 1) * hd;  // from the end of a row to the same row of the next frame
  int kc = 0;  // chunk of the frame the pointers stand on

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  bf16x8 a0[8], b0[8], a1[8], b1[8];
  auto load = [&](bf16x8(&a)[8], bf16x8(&b)[8]) {  // the chunk the pointers stand on, then on to the next
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      a[c] = *reinterpret_cast<const bf16x8*>(pa + c * 8);
      b[c] = *reinterpret_cast<const bf16x8*>(pb + c * 8);
    }
    pa += FW_KC;
    pb += FW_KC;
    if (++kc == cpf) {
      kc = 0;
      pa += skip_a;
      pb += skip_b;
    }
  };
  auto mma = [&](const bf16x8(&a)[8], const bf16x8(&b)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[c], b[c], acc, 0, 0, 0);
  };
  if (nc > 0) load(a0, b0);
  for (int i = 0; i < nc; i += 2) {
    if (i + 1 < nc) load(a1, b1);
    mma(a0, b0);
    if (i + 2 < nc) load(a0, b0);
    if (i + 1 < nc) mma(a1, b1);
  }
  // C lane layout: column n = lq, rows m = 8g + 4h + j in register 4g + j
  float* o = out + (long)slice * ra * rb;
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(long)(m0 + 8 * g + 4 * lh + r) * rb + n0 + lq] = acc[4 * g + r];
}

// out[n] = sum of the `slices` partial tiles ws[s][n], in a fixed order: thread group g (of FW_SG) adds slices g, g + FW_SG, ... in rising
// order, then the FW_SG group sums are added in rising g.  One workgroup = FW_SG groups x 16 float4 columns
constexpr int FW_SG = 16;
__global__ __launch_bounds__(256) void facmat_factor_sum_kernel(const float* __restrict__ ws, float* __restrict__ out, int n4, int slices) {
  __shared__ float4v part[FW_SG][16];
  const int col = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + col;  // float4 index; n4 is a multiple of 16 (Ra * Rb / 4 with Ra, Rb multiples of 64)
  const long stride = (long)n4 * 4;
  float4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int sl = g; sl < slices; sl += FW_SG) acc += *reinterpret_cast<const float4v*>(ws + sl * stride + (long)i * 4);
  part[g][col] = acc;
  __syncthreads();
  if (g == 0) {
    float4v t = part[0][col];
#pragma unroll
    for (int k = 1; k < FW_SG; ++k) t += part[k][col];
    *reinterpret_cast<float4v*>(out + (long)i * 4) = t;
  }
}

}  // namespace

// Slices of the frame axis for one call: one workgroup per CU over the 1, 2 or 4 output tiles, at most one slice per frame and at most
// `max_slices` (what the caller's workspace holds: slices * Ra * Rb floats).  A function of the shape and the device alone.
int facmat_factor_wgrad_slices(int frames, int ra, int rb, long max_slices) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    if (cus < 1) cus = 256;
  }
  const int tiles = (ra / 64) * (rb / 64);
  long slices = tiles > 0 ? cus / tiles : 1;
  if (slices > frames) slices = frames;
  if (slices > max_slices) slices = max_slices;
  return slices < 1 ? 1 : (int)slices;
}

// out [Ra][Rb] fp32; ws: workspace for the slices' partial tiles (ws_floats / (Ra * Rb) bounds the slice count; null: one slice, stored
// straight into out, as with one frame)
int launch_facmat_factor_wgrad(const bf16* a, const bf16* b, float* out, float* ws, size_t ws_floats, int frames, int ra, int rb, int hd,
                               hipStream_t s) {
  DFOT_REQUIRE(a && b && out, DFOT_ERR_ARG, "facmat_factor_wgrad: null pointer");
  DFOT_REQUIRE((ra == 64 || ra == 128) && (rb == 64 || rb == 128), DFOT_ERR_SHAPE, "facmat_factor_wgrad: %d x %d output; both sides are 64 or 128",
               ra, rb);
  DFOT_REQUIRE(hd > 0 && hd % FW_KC == 0, DFOT_ERR_SHAPE, "facmat_factor_wgrad: hidden %d must be a positive multiple of %d", hd, FW_KC);
  DFOT_REQUIRE(frames >= 1, DFOT_ERR_SHAPE, "facmat_factor_wgrad: %d frames", frames);
  const int slices = facmat_factor_wgrad_slices(frames, ra, rb, ws ? (long)(ws_floats / ((size_t)ra * rb)) : 1);
  hipLaunchKernelGGL(facmat_factor_wgrad_kernel, dim3(slices, ra / 64, rb / 64), dim3(256), 0, s, a, b, slices == 1 ? out : ws, frames, ra, rb, hd,
                     slices);
  if (slices > 1) hipLaunchKernelGGL(facmat_factor_sum_kernel, dim3(ra * rb / 64), dim3(256), 0, s, ws, out, ra * rb / 4, slices);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace dfot
