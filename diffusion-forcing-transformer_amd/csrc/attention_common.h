// LDS image of a K / V tile shared by the forward attention kernels (attention.hip, attention_v3.hip, attention_v5.hip,
// attention_ks.hip): 64 keys x D elements, rows unpadded, the 16-byte chunks of a row XOR-swizzled against bank conflicts: swz_k
// for the row reads of K (ds_read_b128), swz_v for the transposed reads of V (ds_read_b64_tr_b16).  The swizzles are involutions,
// so the LDS-DMA kernels apply them to the per-lane SOURCE chunk.  (The backward kernels and wgrad.hip keep their own images.)
#pragma once
#include "common.h"

namespace dfot {

template <int D>
struct AttnCfg {
  static constexpr int KV = 64;                  // keys per tile
  static constexpr int ROWB = D * 2;             // bytes per K/V row in LDS
  static constexpr int TILE = KV * ROWB;         // bytes of one K or V tile
  static constexpr int CH = D / 8;               // 16-byte chunks per row
  static constexpr int PER_THREAD = KV * CH / 256;
  __device__ static int swz_k(int row, int c) { return D == 64 ? (c ^ ((row >> 1) & 7)) : (c ^ (row & 15)); }
  __device__ static int swz_v(int row, int c) { return D == 64 ? (c ^ (((row >> 1) & 1) << 2)) : (c ^ ((row & 3) << 2)); }
};

// V^T fragment (A operand of O^T += V^T P^T) of the V tile `sv` for head-dim block dvt (32 columns) and the 16 keys of step (kt2, s),
// by the builtin form of the transposed read: the 16-lane group gi = lane>>4 reads the 4x16 block rows kb+{0..3}, cols dvt*32 +
// 16*(gi&1) + {0..15}; lane 4q+p of the group supplies row q, columns 4p..4p+3.  For kernels without an LDS-DMA in flight (see
// lds_read_tr16 in common.h for the others).
template <int D>
__device__ __forceinline__ bf16x8 tr_frag_v(const char* sv, int dvt, int kt2, int s, int lane) {
  using C = AttnCfg<D>;
  const int lh = lane >> 5;
  const int kb = kt2 * 32 + 16 * s + 4 * lh;
  const int q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int col = dvt * 32 + 16 * ((lane >> 4) & 1) + 4 * p4;
  const int r0 = kb + q4, r1 = kb + 8 + q4;
  const char* a0 = sv + r0 * C::ROWB + C::swz_v(r0, col >> 3) * 16 + (col & 7) * 2;
  const char* a1 = sv + r1 * C::ROWB + C::swz_v(r1, col >> 3) * 16 + (col & 7) * 2;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a1));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

}  // namespace dfot
