// The finalize-time kernels of the noise-level embedding (run once per weight load), shared by dit.hip (and dit_train.inl inside it)
// and dit1d.hip: sinusoidal features of every level and the fp32 row-times-Linear both embedding MLPs are evaluated with.
#pragma once
#include "common.h"

namespace dfot {
namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): feat[level] = [cos(level*f_i) | sin(level*f_i)]
__global__ void tstep_features_kernel(const float* __restrict__ freqs, float* __restrict__ feat, int levels, int dim) {
  const int half = dim / 2;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)levels * dim) return;
  const int lv = (int)(i / dim), c = (int)(i % dim);
  const float a = __fmul_rn((float)lv, freqs[c < half ? c : c - half]);
  feat[i] = c < half ? cosf(a) : sinf(a);
}

// v = act(b[o] + sum_k W[o][k] * in[r][k]); one wave per (o, r); ACT: 0 none, 1 SiLU; out (optional) = v, out_silu_bf16 (optional) =
// bf16(SiLU(v))
template <int ACT>
__global__ __launch_bounds__(256) void rows_linear_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ out,
                                                          bf16* __restrict__ out_silu_bf16, int kdim, int odim) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o = blockIdx.x * 4 + wave;
  const long r = blockIdx.y;
  if (o >= odim) return;
  float acc = 0.f;
  for (int i = lane; i < kdim; i += 64) acc += w[(long)o * kdim + i] * in[r * kdim + i];
  acc = wave_sum(acc);
  if (lane == 0) {
    float v = acc + b[o];
    if (ACT == 1) v = silu_f(v);
    if (out) out[r * odim + o] = v;
    if (out_silu_bf16) out_silu_bf16[r * odim + o] = f2bf(silu_f(v));
  }
}

}  // namespace
}  // namespace dfot
