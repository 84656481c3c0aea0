// Training kernels of the DiT1D backbone (share_norm blocks, dit1d.hip): what the backward of the model needs beyond the row-wise kernels
// it shares with the DiT3D trainers (dit_train.inl).  All fp32, no atomics, every sum in a fixed order: two runs give the same bits.
//
// A share_norm block keeps the UNMODULATED normalised row as its residual base,
//     n = LN(x) ;  m = n (1 + scale) + shift ;  x' = n + gate * f(m)
// so the LayerNorm's backward receives two gradients: dres over the residual path (it reaches n directly) and dm from the GEMM that
// consumed m (it reaches n through (1 + scale), and it alone feeds dshift and dscale):
//     dn = dres + dm (1 + scale) ;  dshift[frame] = sum_rows dm ;  dscale[frame] = sum_rows dm n ;
//     dx = rstd (dn - mean(dn) - n mean(dn n))
// The DiT3D blocks of dit_train.inl add onto the MODULATED row, so their ln_bwd has one incoming gradient that takes every one of these
// paths; used here it would push dres through (1 + scale) and into dshift / dscale.
//
// Rows are processed one wave each in the layout of dit1d.hip's d1_ln_row: lane l holds channels (i * 64 + l) * 4 .. + 3 of chunk i,
// hidden a multiple of 64, <= 2048 (up to eight chunks, the dead ones skipped).
#include "dit1d_train.h"
#include "level_embed.h"  // wave_sum

namespace dfot {
namespace {

typedef __attribute__((ext_vector_type(4))) float float4v;
constexpr int D1_MAX_CHUNKS = 8;

__device__ __forceinline__ float sum4(float4v v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ float dot4(float4v a, float4v b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }

// d1_ln_row of dit1d.hip (the same operations in the same order, so N has the bits of the inference kernel's rows) that also returns the
// statistics: v <- (x - mean) * rstd
__device__ __forceinline__ void d1_ln_row_stats(const float* __restrict__ xr, int hidden, float eps, int lane, float4v (&v)[D1_MAX_CHUNKS],
                                                float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = float4v{0.f, 0.f, 0.f, 0.f};
    if (c < hidden) v[i] = *reinterpret_cast<const float4v*>(xr + c);
    s += sum4(v[i]);
  }
  mean = wave_sum(s) / (float)hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < hidden) {
      v[i] -= mean;
      q += dot4(v[i], v[i]);
    }
  }
  rstd = rsqrtf(wave_sum(q) / (float)hidden + eps);
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) v[i] *= rstd;
}

// share_norm LayerNorm of the training forward, not in place: N[row] = LN(X[row]) (fp32: saved, and the base of the gated step that
// follows), rstd[row] (saved), M[row] = bf16(N (1 + scale) + shift) with the frame's own (shift | scale) = table[frame][off .. off + 2 hidden)
__global__ __launch_bounds__(256) void d1_ln_share_train_kernel(const float* __restrict__ X, float* __restrict__ N, float* __restrict__ rstd_out,
                                                                bf16* __restrict__ M, const float* __restrict__ table, long ldt, long off,
                                                                int hidden, int rows_per_frame, int rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4v v[D1_MAX_CHUNKS];
  float mean, rstd;
  d1_ln_row_stats(X + (long)row * hidden, hidden, eps, lane, v, mean, rstd);
  const float* sh = table + (long)(row / rows_per_frame) * ldt + off;
  const float* sc = sh + hidden;
  float* nr = N + (long)row * hidden;
  bf16* mr = M + (long)row * hidden;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < hidden) {
      *reinterpret_cast<float4v*>(nr + c) = v[i];
      const float4v a = *reinterpret_cast<const float4v*>(sh + c);
      const float4v g = *reinterpret_cast<const float4v*>(sc + c);
      const float4v m = v[i] * (1.0f + g) + a;
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bf(m[j]);
      *reinterpret_cast<bf16x4*>(mr + c) = o;
    }
  }
  if (lane == 0) rstd_out[row] = rstd;
}

// the four waves' per-lane sums -> LDS [4][hidden] -> one plane row of dmod_part, added in a fixed order
__device__ __forceinline__ void d1_store_plane(const float4v (&acc)[D1_MAX_CHUNKS], float* red, float* __restrict__ out, int hidden, int lane,
                                               int wave) {
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < hidden) *reinterpret_cast<float4v*>(red + wave * hidden + c) = acc[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < hidden; c += 256) out[c] = (red[c] + red[hidden + c]) + (red[2 * hidden + c] + red[3 * hidden + c]);
  __syncthreads();
}

// Backward of the share_norm LayerNorm, one launch: workgroup (frame, plane) owns rows [plane * per, (plane + 1) * per) of the frame,
// per = rows_per_frame / 4; wave w takes rows w, w + 4, ... of them, writes their dx and keeps the lane's share of dshift / dscale in
// registers; the four waves' sums meet in LDS and leave as plain stores into the workgroup's own plane of dmod_part.
// MOD == false is the final layer's LayerNorm: dn = dres, no dm, no table, no dmod_part.  dx may be dres (a row is read whole before it is
// written, by the one wave that owns it).
template <bool MOD>
__global__ __launch_bounds__(256) void d1_ln_share_bwd_kernel(const float* dres, const float* __restrict__ dm, const float* __restrict__ N,
                                                              const float* __restrict__ rstd, const float* __restrict__ table, long ldt,
                                                              long off, float* dx, float* __restrict__ dmod_part, int hidden,
                                                              int rows_per_frame) {
  extern __shared__ float red[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long frame = blockIdx.x;
  const int per = rows_per_frame / D1_DMOD_PLANES, r0 = blockIdx.y * per;
  const float inv = 1.0f / (float)hidden;
  float4v sc1[D1_MAX_CHUNKS], ash[D1_MAX_CHUNKS], asc[D1_MAX_CHUNKS];
  if (MOD) {
    const float* sc = table + frame * ldt + off + hidden;
#pragma unroll
    for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
      const int c = (i * 64 + lane) * 4;
      sc1[i] = ash[i] = asc[i] = float4v{0.f, 0.f, 0.f, 0.f};
      if (c < hidden) sc1[i] = 1.0f + *reinterpret_cast<const float4v*>(sc + c);
    }
  }
  for (int r = r0 + wave; r < r0 + per; r += 4) {
    const long row = frame * rows_per_frame + r, base = row * hidden;
    float4v n[D1_MAX_CHUNKS], g[D1_MAX_CHUNKS];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
      const int c = (i * 64 + lane) * 4;
      n[i] = g[i] = float4v{0.f, 0.f, 0.f, 0.f};
      if (c < hidden) {
        n[i] = *reinterpret_cast<const float4v*>(N + base + c);
        g[i] = *reinterpret_cast<const float4v*>(dres + base + c);
        if (MOD) {
          const float4v d = *reinterpret_cast<const float4v*>(dm + base + c);
          g[i] += d * sc1[i];
          ash[i] += d;
          asc[i] += d * n[i];
        }
      }
      s1 += sum4(g[i]);
      s2 += dot4(g[i], n[i]);
    }
    s1 = wave_sum(s1) * inv;
    s2 = wave_sum(s2) * inv;
    const float rs = rstd[row];
#pragma unroll
    for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < hidden) *reinterpret_cast<float4v*>(dx + base + c) = (g[i] - s1 - n[i] * s2) * rs;
    }
  }
  if (MOD) {
    float* o = dmod_part + ((long)blockIdx.y * gridDim.x + frame) * ldt + off;
    d1_store_plane(ash, red, o, hidden, lane, wave);
    d1_store_plane(asc, red, o + hidden, hidden, lane, wave);
  }
}

// Final layer backward, data part (forward: out[(frame, c, l)] = sum_h nf[row][h] W[c][h] + b[c], nf = LN(X[row]) without affine):
// d nf = sum_c d_out[(frame, c, l)] W[c][:] stays in registers and goes straight through the LayerNorm backward; stats[row] = (mean, rstd)
// for the weight gradient.  One wave per token row.
__global__ __launch_bounds__(256) void d1_final_dgrad_kernel(const float* __restrict__ dout, const float* __restrict__ X, const float* __restrict__ w,
                                                             float* __restrict__ dx, float* __restrict__ stats, int hidden, int C, int L, int rows,
                                                             float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4v v[D1_MAX_CHUNKS], g[D1_MAX_CHUNKS];
  float mean, rstd;
  d1_ln_row_stats(X + (long)row * hidden, hidden, eps, lane, v, mean, rstd);
  const long frame = row / L;
  const int l = row % L;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) g[i] = float4v{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const float d = dout[(frame * C + c) * L + l];
    const float* wr = w + (long)c * hidden;
#pragma unroll
    for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
      const int ch = (i * 64 + lane) * 4;
      if (ch < hidden) g[i] += d * *reinterpret_cast<const float4v*>(wr + ch);
    }
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    s1 += sum4(g[i]);
    s2 += dot4(g[i], v[i]);
  }
  s1 = wave_sum(s1) / (float)hidden;
  s2 = wave_sum(s2) / (float)hidden;
  float* orow = dx + (long)row * hidden;
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int ch = (i * 64 + lane) * 4;
    if (ch < hidden) *reinterpret_cast<float4v*>(orow + ch) = (g[i] - s1 - v[i] * s2) * rstd;
  }
  if (lane == 0) {
    stats[2 * (long)row] = mean;
    stats[2 * (long)row + 1] = rstd;
  }
}

// First stage of the two weight gradients, both sums over the token rows of (a row-major operand) x (a value gathered from a channel-major
// frame):  part[chunk][c][h] = sum over the chunk's rows of a[row][h] * y[(frame, c, l)], one thread per (h, c), D1_SUM_ROWS rows per chunk.
//   FINAL: a = (X - mean) rstd, y = d_out: dW of the final Linear [C][hidden]; bias part[chunk][c] = sum of y
//   else:  a = dX0,             y = x:     dW of the token embedding, transposed; bias part[chunk][h] = sum of a
template <bool FINAL>
__global__ __launch_bounds__(256) void d1_outer_part_kernel(const float* __restrict__ a, const float* __restrict__ stats, const float* __restrict__ y,
                                                            float* __restrict__ part, float* __restrict__ bpart, int C, int L, int hidden,
                                                            long rows) {
  const int h = blockIdx.y * 256 + threadIdx.x;
  if (h >= hidden) return;
  const int c = blockIdx.z;
  const long chunk = blockIdx.x, r0 = chunk * D1_SUM_ROWS;
  const long r1 = r0 + D1_SUM_ROWS < rows ? r0 + D1_SUM_ROWS : rows;
  float acc = 0.f, bacc = 0.f;
  for (long r = r0; r < r1; ++r) {
    const long frame = r / L;
    const int l = (int)(r % L);
    const float s = y[(frame * C + c) * L + l];
    float av = a[r * hidden + h];
    if (FINAL) av = (av - stats[2 * r]) * stats[2 * r + 1];
    acc += av * s;
    bacc += FINAL ? s : av;
  }
  part[(chunk * C + c) * hidden + h] = acc;
  if (FINAL) {
    if (h == 0) bpart[chunk * C + c] = bacc;
  } else {
    if (c == 0) bpart[chunk * hidden + h] = bacc;
  }
}
// Second stage: the chunks added in their order.  dW[c][h] (transpose == 0) or dW[h][c]; db [nb]
__global__ void d1_outer_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bpart, float* __restrict__ dW, float* __restrict__ db,
                                       int C, int hidden, int nb, int nchunks, int transpose) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, n = (long)C * hidden;
  if (i < n) {
    float acc = 0.f;
    for (int k = 0; k < nchunks; ++k) acc += part[k * n + i];
    const long c = i / hidden, h = i % hidden;
    dW[transpose ? h * C + c : i] = acc;
  } else if (i < n + nb) {
    const long j = i - n;
    float acc = 0.f;
    for (int k = 0; k < nchunks; ++k) acc += bpart[(long)k * nb + j];
    db[j] = acc;
  }
}

// Token embedding backward, input part: dx[(frame, c, l)] = sum_h dX0[row][h] W[h][c].  One wave per token row; every dx element has one row.
__global__ __launch_bounds__(256) void d1_tok_embed_dgrad_kernel(const float* __restrict__ dX0, const float* __restrict__ w, float* __restrict__ dx,
                                                                 int C, int L, int hidden, long rows) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float4v d[D1_MAX_CHUNKS];
#pragma unroll
  for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
    const int ch = (i * 64 + lane) * 4;
    d[i] = float4v{0.f, 0.f, 0.f, 0.f};
    if (ch < hidden) d[i] = *reinterpret_cast<const float4v*>(dX0 + row * hidden + ch);
  }
  const long frame = row / L;
  const int l = (int)(row % L);
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < D1_MAX_CHUNKS; ++i) {
      const int ch = (i * 64 + lane) * 4;
      if (ch < hidden) {
        const float* wp = w + (long)ch * C + c;
        acc += (d[i][0] * wp[0] + d[i][1] * wp[C]) + (d[i][2] * wp[2 * C] + d[i][3] * wp[3 * C]);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) dx[(frame * C + c) * L + l] = acc;
  }
}

template <bool FINAL>
int launch_d1_outer(const float* a, const float* stats, const float* y, float* part, float* dW, float* db, int C, int L, int hidden, long rows,
                    hipStream_t s) {
  const int nchunks = cdiv(rows, D1_SUM_ROWS), nb = FINAL ? C : hidden;
  float* bpart = part + (size_t)nchunks * C * hidden;
  hipLaunchKernelGGL(d1_outer_part_kernel<FINAL>, dim3(nchunks, cdiv(hidden, 256), C), dim3(256), 0, s, a, stats, y, part, bpart, C, L, hidden, rows);
  DFOT_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(d1_outer_reduce_kernel, dim3(cdiv((long)C * hidden + nb, 256)), dim3(256), 0, s, part, bpart, dW, db, C, hidden, nb, nchunks,
                     FINAL ? 0 : 1);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace

int launch_d1_ln_share_train(const float* X, float* N, float* rstd, bf16* M, const float* table, long ldt, long off, int hidden, int rows_per_frame,
                             int rows, float eps, hipStream_t s) {
  hipLaunchKernelGGL(d1_ln_share_train_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, X, N, rstd, M, table, ldt, off, hidden, rows_per_frame, rows,
                     eps);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
int launch_d1_ln_share_bwd(const float* dres, const float* dm, const float* N, const float* rstd, const float* table, long ldt, long off, float* dx,
                           float* dmod_part, int hidden, int rows_per_frame, int frames, hipStream_t s) {
  const dim3 grid(frames, D1_DMOD_PLANES);
  if (dm)
    hipLaunchKernelGGL(d1_ln_share_bwd_kernel<true>, grid, dim3(256), 4 * hidden * sizeof(float), s, dres, dm, N, rstd, table, ldt, off, dx,
                       dmod_part, hidden, rows_per_frame);
  else
    hipLaunchKernelGGL(d1_ln_share_bwd_kernel<false>, grid, dim3(256), 0, s, dres, dm, N, rstd, table, ldt, off, dx, dmod_part, hidden,
                       rows_per_frame);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
int launch_d1_final_dgrad(const float* dout, const float* X, const float* w, float* dx, float* stats, int hidden, int C, int L, int rows, float eps,
                          hipStream_t s) {
  hipLaunchKernelGGL(d1_final_dgrad_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, dout, X, w, dx, stats, hidden, C, L, rows, eps);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}
int launch_d1_final_wgrad(const float* dout, const float* X, const float* stats, float* part, float* dW, float* db, int hidden, int C, int L, long rows,
                          hipStream_t s) {
  return launch_d1_outer<true>(X, stats, dout, part, dW, db, C, L, hidden, rows, s);
}
int launch_d1_tok_embed_wgrad(const float* dX0, const float* x, float* part, float* dW, float* db, int C, int L, int hidden, long rows, hipStream_t s) {
  return launch_d1_outer<false>(dX0, nullptr, x, part, dW, db, C, L, hidden, rows, s);
}
int launch_d1_tok_embed_dgrad(const float* dX0, const float* w, float* dx, int C, int L, int hidden, long rows, hipStream_t s) {
  hipLaunchKernelGGL(d1_tok_embed_dgrad_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, dX0, w, dx, C, L, hidden, rows);
  DFOT_CHECK_HIP(hipGetLastError());
  return DFOT_OK;
}

}  // namespace dfot

using namespace dfot;

// ---- single launches (test entries: the launchers above on caller-provided buffers) ----
static int op_d1t_shape(const char* what, int hidden, int C, int L, int64_t rows) {
  DFOT_REQUIRE(hidden > 0 && hidden % 64 == 0 && hidden <= 2048, DFOT_ERR_SHAPE, "%s: hidden %d must be a multiple of 64, <= 2048", what, hidden);
  DFOT_REQUIRE(C > 0 && C <= 64, DFOT_ERR_SHAPE, "%s: in_channels %d must be in [1, 64]", what, C);
  DFOT_REQUIRE(L > 0 && rows > 0 && rows % L == 0 && rows * (int64_t)hidden < (1LL << 31), DFOT_ERR_SHAPE,
               "%s: %ld rows of %d per frame (rows x hidden must stay below 2^31)", what, (long)rows, L);
  return DFOT_OK;
}

extern "C" {

int dfot_op_dit1d_ln_share_train(const float* X, float* N, float* rstd, void* M, const float* table, int64_t ldt, int64_t off, int hidden,
                                 int rows_per_frame, int rows, float eps, void* stream) {
  DFOT_REQUIRE(X && N && rstd && M && table, DFOT_ERR_ARG, "dit1d ln_share_train: null argument");
  if (int rc = op_d1t_shape("dit1d ln_share_train", hidden, 1, rows_per_frame, rows)) return rc;
  DFOT_REQUIRE(off >= 0 && off % 4 == 0 && ldt % 4 == 0 && ldt >= off + 2L * hidden && eps > 0.f, DFOT_ERR_ARG,
               "dit1d ln_share_train: table row of %ld with (shift | scale) at %ld (multiples of 4), eps %g", (long)ldt, (long)off, eps);
  return launch_d1_ln_share_train(X, N, rstd, (bf16*)M, table, ldt, off, hidden, rows_per_frame, rows, eps, (hipStream_t)stream);
}

int dfot_op_dit1d_ln_share_bwd(const float* dres, const float* dm, const float* N, const float* rstd, const float* table, int64_t ldt, int64_t off,
                               float* dx, float* dmod_part, int hidden, int rows_per_frame, int frames, void* stream) {
  DFOT_REQUIRE(dres && N && rstd && dx && (!dm || (table && dmod_part)), DFOT_ERR_ARG, "dit1d ln_share_bwd: null argument");
  DFOT_REQUIRE(frames > 0 && frames <= (1 << 20), DFOT_ERR_SHAPE, "dit1d ln_share_bwd: %d frames", frames);
  DFOT_REQUIRE(rows_per_frame > 0 && rows_per_frame <= (1 << 20) && rows_per_frame % D1_DMOD_PLANES == 0, DFOT_ERR_SHAPE,
               "dit1d ln_share_bwd: rows_per_frame %d must be a multiple of %d", rows_per_frame, D1_DMOD_PLANES);
  if (int rc = op_d1t_shape("dit1d ln_share_bwd", hidden, 1, rows_per_frame, (int64_t)frames * rows_per_frame)) return rc;
  DFOT_REQUIRE(!dm || (off >= 0 && off % 4 == 0 && ldt % 4 == 0 && ldt >= off + 2L * hidden), DFOT_ERR_ARG,
               "dit1d ln_share_bwd: table row of %ld with (shift | scale) at %ld (multiples of 4)", (long)ldt, (long)off);
  return launch_d1_ln_share_bwd(dres, dm, N, rstd, table, ldt, off, dx, dmod_part, hidden, rows_per_frame, frames, (hipStream_t)stream);
}

int dfot_op_dit1d_final_bwd(const float* dout, const float* X, const float* w, float* dx, float* stats, float* part, float* dW, float* db, int hidden,
                            int C, int L, int rows, float eps, void* stream) {
  DFOT_REQUIRE(dout && X && w && dx && stats && part && dW && db, DFOT_ERR_ARG, "dit1d final_bwd: null argument");
  if (int rc = op_d1t_shape("dit1d final_bwd", hidden, C, L, rows)) return rc;
  DFOT_REQUIRE(eps > 0.f, DFOT_ERR_ARG, "dit1d final_bwd: eps must be positive");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_d1_final_dgrad(dout, X, w, dx, stats, hidden, C, L, rows, eps, s)) return rc;
  return launch_d1_final_wgrad(dout, X, stats, part, dW, db, hidden, C, L, rows, s);
}

int dfot_op_dit1d_tok_embed_wgrad(const float* dX0, const float* x, float* part, float* dW, float* db, int C, int L, int hidden, int64_t rows,
                                  void* stream) {
  DFOT_REQUIRE(dX0 && x && part && dW && db, DFOT_ERR_ARG, "dit1d tok_embed_wgrad: null argument");
  if (int rc = op_d1t_shape("dit1d tok_embed_wgrad", hidden, C, L, rows)) return rc;
  return launch_d1_tok_embed_wgrad(dX0, x, part, dW, db, C, L, hidden, (long)rows, (hipStream_t)stream);
}

int dfot_op_dit1d_tok_embed_dgrad(const float* dX0, const float* w, float* dx, int C, int L, int hidden, int64_t rows, void* stream) {
  DFOT_REQUIRE(dX0 && w && dx, DFOT_ERR_ARG, "dit1d tok_embed_dgrad: null argument");
  if (int rc = op_d1t_shape("dit1d tok_embed_dgrad", hidden, C, L, rows)) return rc;
  return launch_d1_tok_embed_dgrad(dX0, w, dx, C, L, hidden, (long)rows, (hipStream_t)stream);
}

}  // extern "C"
