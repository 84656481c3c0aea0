// Launchers of the DiT1D training kernels (dit1d_train.hip): the share_norm LayerNorm with saved statistics and its backward, the final
// layer's backward and the token embedding's backward.  Each launch exists once, for a training engine and for the dfot_op_dit1d_* entries.
#pragma once
#include "common.h"

namespace dfot {

constexpr int D1_DMOD_PLANES = 4;  // planes of dmod_part [planes][frames][ldt]: the layout (and TR_CHUNKS) of dit_train.inl
constexpr int D1_SUM_ROWS = 64;    // rows per partial sum of the two weight gradients

// floats of the partial-sum workspace of launch_d1_final_wgrad (nb = C) / launch_d1_tok_embed_wgrad (nb = hidden)
inline size_t d1_wgrad_part_floats(long rows, int C, int hidden, int nb) {
  return (size_t)cdiv(rows, D1_SUM_ROWS) * ((size_t)C * hidden + nb);
}

// N = LayerNorm(X) (fp32), rstd [rows], M = bf16(N (1 + scale) + shift), (shift | scale) = table[row / rows_per_frame][off .. off + 2 hidden)
int launch_d1_ln_share_train(const float* X, float* N, float* rstd, bf16* M, const float* table, long ldt, long off, int hidden, int rows_per_frame,
                             int rows, float eps, hipStream_t s);
// dn = dres + dm (1 + scale), dx = rstd (dn - mean(dn) - N mean(dn N)); dshift = sum_rows dm and dscale = sum_rows dm N of every quarter of a
// frame's rows into its plane of dmod_part at columns [off, off + 2 hidden).  dm == nullptr: dn = dres, no table, nothing written to dmod_part.
// dx may be dres.
int launch_d1_ln_share_bwd(const float* dres, const float* dm, const float* N, const float* rstd, const float* table, long ldt, long off, float* dx,
                           float* dmod_part, int hidden, int rows_per_frame, int frames, hipStream_t s);
// dx = LayerNorm backward of d nf = d_out W (never stored), stats [rows][2] = (mean, rstd) of X's rows
int launch_d1_final_dgrad(const float* dout, const float* X, const float* w, float* dx, float* stats, int hidden, int C, int L, int rows, float eps,
                          hipStream_t s);
// dW [C][hidden] = sum_rows d_out nf, db [C] = sum_rows d_out, nf = (X - mean) rstd from the stats of launch_d1_final_dgrad
int launch_d1_final_wgrad(const float* dout, const float* X, const float* stats, float* part, float* dW, float* db, int hidden, int C, int L, long rows,
                          hipStream_t s);
// dW [hidden][C] = sum_rows dX0 x, db [hidden] = sum_rows dX0
int launch_d1_tok_embed_wgrad(const float* dX0, const float* x, float* part, float* dW, float* db, int C, int L, int hidden, long rows, hipStream_t s);
// dx [frames][C][L] = dX0 W
int launch_d1_tok_embed_dgrad(const float* dX0, const float* w, float* dx, int C, int L, int hidden, long rows, hipStream_t s);

// dit1d.hip: the inference engine's token embedding (X = w x + b + pos) and final layer (LayerNorm + Linear into (B, T, C, 1, L))
int d1_tok_embed(const float* x, const float* w, const float* b, const float* pos, float* X, int C, int L, int n, int hidden, long rows, hipStream_t s);
int d1_final(const float* X, const float* w, const float* b, float* out, int hidden, int C, int L, int rows, float eps, hipStream_t s);

}  // namespace dfot
