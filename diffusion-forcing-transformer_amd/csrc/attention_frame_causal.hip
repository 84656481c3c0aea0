// Frame-causal ("block lower triangular") flash attention forward for the DiT1D backbone (gfx950).
//
// A sequence of n = frames * frame_len tokens; query i attends to key j iff j / frame_len <= i / frame_len: every token of its own and of
// earlier frames, none of later frames (dit1d/dit_model.py:407-427, temporal_causal / video_temporal_causal with no context tokens).
//
// Operands, products and pipeline are those of attention.hip's attn_kernel_v2 (transposed products with the query index on the MFMA lane,
// lane-local online-softmax statistics, K/V tiles by LDS-DMA into a ring, the running max folded into the S^T accumulator, deferred
// rescale, V^T by ds_read_b64_tr_b16), in launch_attention_padded's layout: q, k, v [B][heads][n][dstride] with pad columns zero and q in
// the exp2 domain; DQK / DV are the head-dim sub-ranges actually multiplied.
//
// Tile walk: one workgroup = 4 waves = 128 query rows starting at Q0 (a whole number of frames: frame_len divides 128).  It loops over
// the 64-key tiles t = 0 .. Q0/64 + 1 only, i.e. the keys below Q0 + 128; the tiles above the block diagonal are never loaded.  The
// tiles below Q0 need no mask.  The last two tiles (keys Q0 .. Q0+127) straddle the diagonal: every score there passes through
//     s = (key / frame_len > query / frame_len) ? -inf : s
// BEFORE the row maximum, so a masked key contributes exp2(-inf) = 0 exactly; a select, never a bias.  The select is on registers: every
// lane runs every LDS read (ds_read_b64_tr_b16 needs EXEC all ones).  Key 0 is visible to every query, so the first tile gives every row a
// finite running maximum and no row is ever fully masked.  A wave whose 32 rows end before a tile begins skips that tile's arithmetic; the
// branch is wave-uniform, and the DMA issue, the waits and the barriers stay outside it.
//
// Workgroup order: (batch, head)-major per XCD as in attn_kernel_v2 (the query tiles of a head share K/V in one L2), and inside a head
// the heaviest query tile (largest Q0, most key tiles) first.
// Summation order: a function of (n, frame_len, d) and the query tile only -- no atomics, no key split, no dependence on the batch or on
// later frames' data (their tiles are not read; inside the diagonal tiles they are selected away before the maximum and the sums).
#include "attention_common.h"
#include "dfot_hip.h"
#include "kernels.h"

namespace dfot {

// LSE (training): the kernel also leaves the log2-domain log-sum-exp of every query row, lse[(b * heads + head) * N + row] = m + log2(l),
// which attention_bwd.hip's frame-causal kernels consume.  A compile-time parameter: the inference instantiation carries no test of it.
template <int D, int NST, int DQK, int DV, bool LSE>
__global__ __launch_bounds__(256) void attn_frame_causal_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                                const bf16* __restrict__ V, bf16* __restrict__ O, long ldo, int N,
                                                                int heads, int flog, int ohs, int dvalid, float* __restrict__ lse) {
  static_assert(DQK % 16 == 0 && DV % 32 == 0 && DQK <= D && DV <= D, "head-dim sub-range");
  using C = AttnCfg<D>;
  constexpr float THR = 8.0f;
  constexpr int RPI = 1024 / C::ROWB;        // rows covered by one 1-KiB DMA instruction (8 or 4)
  constexpr int IPW = (C::TILE / 1024) / 4;  // DMA instructions per wave per tile (2 or 4)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, lh = lane >> 5;
  const int qtiles = N / 128;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lin / qtiles;
  const int Q0 = (qtiles - 1 - lin % qtiles) * 128;  // heaviest query tile of a head first
  const long base = (long)bh * N * D;
  const int q0 = Q0 + wave * 32;
  const bf16* Qb = Q + base;
  const bf16* Kb = K + base;
  const bf16* Vb = V + base;
  const int qframe = (q0 + lq) >> flog;                     // this lane's query frame
  const int wave_keys = (((q0 + 31) >> flog) + 1) << flog;  // keys this wave's rows can see: [0, wave_keys)

  bf16x8 qf[DQK / 16];
  const bf16* qrow = Qb + (long)(q0 + lq) * D + lh * 8;
#pragma unroll
  for (int ks = 0; ks < DQK / 16; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + ks * 16);

  // per-lane DMA source offsets (elements) within a tile: LDS position (row, pos) receives source chunk swz(row,pos)
  int koff[IPW], voff[IPW];
#pragma unroll
  for (int i = 0; i < IPW; ++i) {
    const int inst = wave * IPW + i;
    const int row = inst * RPI + lane / C::CH;
    const int pos = lane % C::CH;
    koff[i] = row * D + C::swz_k(row, pos) * 8;
    voff[i] = row * D + C::swz_v(row, pos) * 8;
  }
  auto issue = [&](int t, int stage) {
    char* sk = smem + stage * 2 * C::TILE;
    char* sv = sk + C::TILE;
    const bf16* kt = Kb + (long)t * C::KV * D;
    const bf16* vt = Vb + (long)t * C::KV * D;
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
      const int inst = wave * IPW + i;
      __builtin_amdgcn_global_load_lds(DFOT_GLOBAL_PTR(kt + koff[i]), DFOT_LDS_PTR(sk + inst * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(DFOT_GLOBAL_PTR(vt + voff[i]), DFOT_LDS_PTR(sv + inst * 1024), 16, 0, 0);
    }
  };

  f32x16 oacc[DV / 32];
#pragma unroll
  for (int i = 0; i < DV / 32; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
  float m_run = 0.f, l_i = 0.f;

  const int nt = (Q0 + 128) / C::KV;  // key tiles below the end of this workgroup's last frame: 2 .. N / KV
  const int diag = Q0 / C::KV;        // first tile that straddles the block diagonal
  // NST == 2: tile t+1 is loaded while t is computed (vmcnt(0) + barrier per tile).  NST == 3: tile t+2 stays in flight across the
  // barrier; the wait before the barrier is counted (2*IPW loads of the newest tile may be outstanding).  nt >= 2 always.
  issue(0, 0);
  if constexpr (NST == 3) {
    issue(1, 1);
    if constexpr (IPW == 2) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const char* sk = smem + cur * 2 * C::TILE;
    const char* sv = sk + C::TILE;
    if constexpr (NST == 3) {
      if (t + 2 < nt) issue(t + 2, cur == 0 ? 2 : cur - 1);
    } else {
      if (t + 1 < nt) issue(t + 1, cur ^ 1);
    }

    if (t * C::KV < wave_keys) {  // wave-uniform: some row of this wave sees some key of the tile (always true for t = 0)
      // ---- S^T - m = K Q^T - m ----
      f32x16 sacc[2];
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[kt2][r] = -m_run;
        const int row = kt2 * 32 + lq;
#pragma unroll
        for (int ks = 0; ks < DQK / 16; ++ks) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sk + row * C::ROWB + C::swz_k(row, ks * 2 + lh) * 16);
          sacc[kt2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc[kt2], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- frame-causal mask on the diagonal tiles: register r of sub-tile kt2 is key 64t + 32kt2 + 8(r>>2) + 4lh + (r&3) ----
      if (t >= diag) {  // workgroup-uniform
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = t * C::KV + kt2 * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
            sacc[kt2][r] = (key >> flog) > qframe ? -INFINITY : sacc[kt2][r];
          }
      }

      // ---- row max of (s - m) over this lane's 32 keys and the partner half ----
      float mx = fmaxf(fmaxf(sacc[0][0], sacc[0][1]), sacc[0][2]);
#pragma unroll
      for (int r = 3; r < 15; r += 2) mx = fmaxf(fmaxf(mx, sacc[0][r]), sacc[0][r + 1]);
      mx = fmaxf(mx, sacc[0][15]);
#pragma unroll
      for (int r = 0; r < 16; r += 2) mx = fmaxf(fmaxf(mx, sacc[1][r]), sacc[1][r + 1]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));

      // first tile: adopt the max outright (finite: key 0 is visible to every query); later: only when it grew by more than THR.
      // A row whose keys of this tile are all masked has mx = -inf and never asks for a rescale.  The decision and the shift are
      // LANE-LOCAL (a query's two lanes hold the same mx): the wave-wide vote only skips the block when no row grew, and a row that did
      // not grow takes delta = 0, alpha = 1, which changes none of its bits.  A wave's 32 rows are two frames at frame_len 16; a shift
      // decided by the vote (attn_kernel_v2's fmaxf(mx, 0)) would let rows of the later frame change the rounding of the earlier one's.
      const bool grow = (t == 0) || (mx > THR);
      if (__any(grow)) {
        const float delta = grow ? mx : 0.f;
        const float alpha = __builtin_amdgcn_exp2f(-delta);  // t == 0: O and l are still zero
        m_run += delta;
        l_i *= alpha;
#pragma unroll
        for (int i = 0; i < DV / 32; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
#pragma unroll
        for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[kt2][r] -= delta;
      }

      float rs = 0.f;
      bf16x8 pf[2][2];
#pragma unroll
      for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float p = __builtin_amdgcn_exp2f(sacc[kt2][8 * s + j]);
            rs += p;
            pf[kt2][s][j] = f2bf(p);
          }
      l_i += rs;

      // ---- O^T += V^T P^T ----
      // V^T fragments by the inline-asm form of the transposed read (lds_read_tr16, common.h: an LDS-DMA is in flight here).  The bank
      // swizzle depends on q4 only, so one base address per lane and 32-column block; (kt2, s, +8) are immediate offsets.
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dvt = 0; dvt < DV / 32; ++dvt) {
        const int q4 = (lane & 15) >> 2, p4 = lane & 3;
        const int col = dvt * 32 + 16 * ((lane >> 4) & 1) + 4 * p4;
        const int r0 = 4 * lh + q4;
        const unsigned va = (unsigned)(size_t)DFOT_LDS_PTR(sv) + r0 * C::ROWB + C::swz_v(r0, col >> 3) * 16 + (col & 7) * 2;
        u32x2 r000 = lds_read_tr16<0 * C::ROWB>(va), r001 = lds_read_tr16<8 * C::ROWB>(va);
        u32x2 r010 = lds_read_tr16<16 * C::ROWB>(va), r011 = lds_read_tr16<24 * C::ROWB>(va);
        u32x2 r100 = lds_read_tr16<32 * C::ROWB>(va), r101 = lds_read_tr16<40 * C::ROWB>(va);
        u32x2 r110 = lds_read_tr16<48 * C::ROWB>(va), r111 = lds_read_tr16<56 * C::ROWB>(va);
        lds_wait(r000, r001, r010, r011, r100, r101, r110, r111);
        oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(r000, r001), pf[0][0], oacc[dvt], 0, 0, 0);
        oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(r010, r011), pf[0][1], oacc[dvt], 0, 0, 0);
        oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(r100, r101), pf[1][0], oacc[dvt], 0, 0, 0);
        oacc[dvt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(r110, r111), pf[1][1], oacc[dvt], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if constexpr (NST == 3) {
      if (t + 2 < nt) {
        if constexpr (IPW == 2) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      }
      cur = cur == 2 ? 0 : cur + 1;
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- normalise and store: lane holds O[q0+lq][dvt*32 + 8*g + 4*lh + {0..3}] in oacc[dvt][4g..4g+3] ----
  const float l_tot = l_i + __shfl_xor(l_i, 32);
  const float inv = 1.0f / l_tot;
  if constexpr (LSE) {
    if (lh == 0) lse[(long)bh * N + q0 + lq] = m_run + __log2f(l_tot);  // one of the row's two lanes
  }
  const int b = bh / heads, hd = bh % heads;
  bf16* orow = O + ((long)b * N + q0 + lq) * ldo + hd * ohs;
#pragma unroll
  for (int dvt = 0; dvt < DV / 32; ++dvt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 o4;
#pragma unroll
      for (int j = 0; j < 4; ++j) o4[j] = f2bf(oacc[dvt][4 * g4 + j] * inv);
      const int c = dvt * 32 + 8 * g4 + 4 * lh;
      if (c < dvalid) *reinterpret_cast<bf16x4*>(orow + c) = o4;
    }
}

template <int D, int NST, int DQK, int DV, bool LSE>
static int launch_fc_t(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, int flog, int d,
                       hipStream_t stream, float* lse) {
  constexpr auto kern = attn_frame_causal_kernel<D, NST, DQK, DV, LSE>;
  const int lds = 2 * NST * AttnCfg<D>::TILE;  // NST stages of (K, V): 48 KiB (D = 64, three stages) or 64 KiB (D = 128, two)
  if (int rc = ensure_dyn_lds<kern>(lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((n / 128) * batch * heads), dim3(256), lds, stream, q, k, v, o, ldo, n, heads, flog, d, d, lse);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
template <int D, int NST, int DQK, int DV>
static int launch_fc(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n, int flog, int d,
                     hipStream_t stream, float* lse) {
  return lse ? launch_fc_t<D, NST, DQK, DV, true>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, lse)
             : launch_fc_t<D, NST, DQK, DV, false>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, nullptr);
}

int launch_attention_frame_causal(const bf16* q, const bf16* k, const bf16* v, bf16* o, long ldo, int batch, int heads, int n,
                                  int frame_len, int d, hipStream_t stream, float* lse) {
  DFOT_REQUIRE(q && k && v && o, DFOT_ERR_ARG, "attention_frame_causal: null pointer");
  DFOT_REQUIRE(frame_len == 16 || frame_len == 32 || frame_len == 64 || frame_len == 128, DFOT_ERR_SHAPE,
               "attention_frame_causal: frame_len %d not in {16, 32, 64, 128}", frame_len);
  DFOT_REQUIRE(n > 0 && n % 128 == 0, DFOT_ERR_SHAPE, "attention_frame_causal: N=%d must be a positive multiple of 128", n);
  DFOT_REQUIRE(d > 0 && d <= 128 && d % 8 == 0, DFOT_ERR_SHAPE, "attention_frame_causal: head dim %d must be a multiple of 8, <= 128", d);
  DFOT_REQUIRE(batch > 0 && heads > 0 && (long)batch * heads * (n / 128) < (1L << 31), DFOT_ERR_SHAPE,
               "attention_frame_causal: batch %d x heads %d x %d query tiles exceeds the grid", batch, heads, n / 128);
  DFOT_REQUIRE(ldo % 8 == 0 && ldo >= (long)heads * d, DFOT_ERR_SHAPE,
               "attention_frame_causal: output row stride %ld must be a multiple of 8 covering heads*d = %d", ldo, heads * d);
  const int flog = frame_len == 16 ? 4 : frame_len == 32 ? 5 : frame_len == 64 ? 6 : 7;
  // ring depths as launch_attention_padded picked them by measurement: three stages at 64-element rows, two at 128
  if (d <= 32) return launch_fc<64, 3, 32, 32>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, lse);
  if (d <= 64) return launch_fc<64, 3, 64, 64>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, lse);
  if (d <= 80) return launch_fc<128, 2, 80, 96>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, lse);
  if (d <= 96) return launch_fc<128, 2, 96, 96>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, lse);
  return launch_fc<128, 2, 128, 128>(q, k, v, o, ldo, batch, heads, n, flog, d, stream, lse);
}

}  // namespace dfot

extern "C" int dfot_op_attention_frame_causal(const void* q, const void* k, const void* v, void* o, int ldo, int batch, int heads, int n,
                                              int frame_len, int d, void* stream) {
  using dfot::bf16;
  return dfot::launch_attention_frame_causal((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, ldo, batch, heads, n, frame_len, d,
                                             (hipStream_t)stream);
}

extern "C" int dfot_op_attention_frame_causal_lse(const void* q, const void* k, const void* v, void* o, int ldo, float* lse, int batch,
                                                  int heads, int n, int frame_len, int d, void* stream) {
  using dfot::bf16;
  DFOT_REQUIRE(lse, DFOT_ERR_ARG, "attention_frame_causal_lse: null lse pointer");
  return dfot::launch_attention_frame_causal((const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, ldo, batch, heads, n, frame_len, d,
                                             (hipStream_t)stream, lse);
}
