// Balanced tail of the forward attention kernels that run in lock-step rounds (attention_v3.hip, attention_v5.hip, attention_ks.hip):
// with S workgroups resident on the device, T query tiles run as floor(T/S) full rounds; the T mod S left-over tiles are split over
// the key axis into `nsplit` segments each (rem * nsplit <= S), so the last round is as full as the others and 1/nsplit as long.
// The segments write fp32 partials (O, m, l) into an AttnScratch; this file plans the split, carves the scratch and merges the partials.
#include "common.h"
#include "dfot_hip.h"
#include "kernels.h"

namespace dfot {

namespace {

constexpr int KV = 64;  // keys per K / V tile of every kernel that splits its tail

// combine the key segments of the left-over tiles: O = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s.  One thread per
// (query row, 4 columns); DCOLS / 4 threads per row.
template <int DCOLS>
__global__ __launch_bounds__(256) void attn_merge_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                         bf16* __restrict__ O, long ldo, int N, int heads, int full_tiles, int nsplit,
                                                         int rem_tiles, int qrows, float* __restrict__ lse) {
  constexpr int TPR = DCOLS / 4;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = gid / TPR;
  const int c4 = (int)(gid % TPR) * 4;
  if (row >= (long)rem_tiles * qrows) return;
  const int lt = (int)(row / qrows), rloc = (int)(row % qrows);
  const int qtiles = N / qrows;
  float mmax = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mmax = fmaxf(mmax, part_ml[((long)(lt * nsplit + s) * qrows + rloc) * 2]);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, l = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const long pr = (long)(lt * nsplit + s) * qrows + rloc;
    const float w = exp2f(part_ml[pr * 2] - mmax);
    l += w * part_ml[pr * 2 + 1];
    const f32x4 o = *reinterpret_cast<const f32x4*>(part_o + pr * DCOLS + c4);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += w * o[j];
  }
  const float inv = 1.0f / l;
  const int tile = full_tiles + lt;
  const int bh = tile / qtiles, b = bh / heads, hd = bh % heads;
  bf16x4 o4;
#pragma unroll
  for (int j = 0; j < 4; ++j) o4[j] = f2bf(acc[j] * inv);
  *reinterpret_cast<bf16x4*>(O + ((long)b * N + (tile % qtiles) * qrows + rloc) * ldo + hd * DCOLS + c4) = o4;
  if (lse && c4 == 0) lse[(long)bh * N + (tile % qtiles) * qrows + rloc] = mmax + __log2f(l);  // training: log2-domain log-sum-exp of the row
}

// Process-wide scratch of the op-level entry points (dfot_op_attention, tools): it only ever GROWS by allocating a new block; the
// blocks it outgrows are kept until the process ends, so a kernel in flight or a captured graph that holds an old pointer stays
// valid (nothing is freed or synchronised on a launch path).  Backbone handles do not use it: they own an AttnScratch sized in
// their reserve() and pass it in, so two handles / streams never share partial rows and a reserve on one model cannot pull the
// buffer from under another model's captured graph.
AttnScratch* attention_default_scratch() {
  static AttnScratch g;
  return &g;
}

}  // namespace

// wgs_per_cu workgroups of qrows query rows are resident per CU (registers: 2 waves per SIMD)
AttnSplit attn_plan_split(int batch, int heads, int n, int qrows, int wgs_per_cu) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  }
  const int slots = wgs_per_cu * cus;
  AttnSplit sp;
  sp.slots = slots;
  sp.tiles = batch * heads * (n / qrows);
  sp.rem = sp.tiles % slots;
  sp.full = sp.tiles - sp.rem;
  sp.nsplit = 1;
  if (sp.rem) {
    const int ntk = n / KV;
    for (int f = 2; f <= 16 && sp.rem * f <= slots; f *= 2)
      if (ntk % f == 0 && ntk / f >= 4) sp.nsplit = f;
  }
  return sp;
}

// one row of dcols + 2 floats (O | m, l) per query row of every key segment
size_t attn_partial_bytes(const AttnSplit& sp, int qrows, int dcols) {
  return sp.nsplit == 1 ? 0 : (size_t)sp.rem * sp.nsplit * qrows * (dcols + 2) * sizeof(float);
}

size_t attention_scratch_bytes(int batch, int heads, int n, int d) {
  if (d == 128) return attention_ks_scratch_bytes(batch, heads, n, d);  // the 8-wave key-split kernel of attention_ks.hip
  if (d != 64 || n % 256 != 0) return 0;  // d = 64: the level-2 kernels (attention_v3 / v5), 256 query rows per workgroup, two per CU
  return attn_partial_bytes(attn_plan_split(batch, heads, n, 256, 2), 256, 64);
}

int attn_partials(const AttnSplit& sp, int qrows, int dcols, float** po, float** pml, AttnScratch* scratch) {
  *po = *pml = nullptr;
  if (sp.nsplit == 1) return DFOT_OK;
  const size_t bytes = attn_partial_bytes(sp, qrows, dcols);
  if (!scratch) {
    scratch = attention_default_scratch();
    if (bytes > scratch->bytes) {  // grow: a NEW block; the old one is deliberately leaked (see above)
      void* p = nullptr;
      DFOT_CHECK_HIP(hipMalloc(&p, bytes));
      scratch->p = reinterpret_cast<float*>(p);
      scratch->bytes = bytes;
    }
  }
  DFOT_REQUIRE(scratch->p && bytes <= scratch->bytes, DFOT_ERR_STATE,
               "attention: key-split scratch of %zu bytes, launch needs %zu (reserve the handle for this batch first)", scratch->bytes, bytes);
  *po = scratch->p;
  *pml = scratch->p + (size_t)sp.rem * sp.nsplit * qrows * dcols;
  return DFOT_OK;
}

int attn_launch_merge(const AttnSplit& sp, int qrows, int dcols, const float* po, const float* pml, bf16* o, long ldo, int n, int heads,
                      hipStream_t stream, float* lse) {
  if (sp.nsplit == 1) return DFOT_OK;
  DFOT_REQUIRE(dcols == 64 || dcols == 128, DFOT_ERR_SHAPE, "attention merge: %d columns not in {64,128}", dcols);
  const dim3 grid(cdiv((long)sp.rem * qrows * (dcols / 4), 256));
  if (dcols == 64)
    hipLaunchKernelGGL(attn_merge_kernel<64>, grid, dim3(256), 0, stream, po, pml, o, ldo, n, heads, sp.full, sp.nsplit, sp.rem, qrows, lse);
  else
    hipLaunchKernelGGL(attn_merge_kernel<128>, grid, dim3(256), 0, stream, po, pml, o, ldo, n, heads, sp.full, sp.nsplit, sp.rem, qrows, lse);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace dfot
