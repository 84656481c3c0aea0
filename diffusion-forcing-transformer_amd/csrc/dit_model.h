// The DiT family described once, on the host, for the inference engine (dit.hip) and the training engine (dit_train.inl): the configuration
// a handle keeps, the geometry derived from it, the tensors of the reference module in state_dict() order (dit3d.py:45-83 ->
// base_backbone.py:35-62, dit_base.py:156-228, dit_blocks.py:266-287,579-601), the trainer's flat layout and the positional tables.
// Plain C++17 without HIP: tests/dit_model_dump.cpp prints it with a host compiler, tests/test_dit_model_host.py holds it to the names the
// reference's own modules recorded.  The engines bind storage to DitTensor::kind; a name is written here and nowhere else.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "dfot_hip.h"

// the configuration a handle keeps: dfot_dit_config plus what dfot_dit_config_f adds to it
struct DitCfg : dfot_dit_config {
  int32_t fourier_noise = 0;
};

inline DitCfg dit_cfg(const dfot_dit_config& base, int32_t fourier_noise = 0) {
  DitCfg c;
  static_cast<dfot_dit_config&>(c) = base;
  c.fourier_noise = fourier_noise;
  return c;
}

namespace dfot {

struct DitGeom {
  int gh = 0, gw = 0, P = 0, d = 0, dstride = 0, kpatch = 0, oc = 0;
  int c_rows = 0;       // label: rows of the embedding table (num_classes, + 1 null class with dropout)
  long ldt = 0;         // row stride (floats) of the modulation table = total modulation outputs
  long mod_final = 0;   // column of the final layer's (shift|scale)
  bool diffm = false, facmat = false, fac = false;  // the difference front end (1) / matrix temporal blocks (1, 3) / temporal DiTBlocks (2)
};

// the geometry without the modulation columns, which the inventory defines (dit_geometry below)
inline DitGeom dit_grid(const DitCfg& c) {
  DitGeom g;
  const int hd = c.hidden_size;
  g.gh = c.height / c.patch_size;
  g.gw = c.width / c.patch_size;
  g.P = g.gh * g.gw;
  g.d = hd / c.num_heads;
  g.dstride = g.d <= 64 ? 64 : 128;  // attention_dstride (kernels.h), restated: this header includes no HIP
  g.kpatch = c.in_channels * c.patch_size * c.patch_size;
  g.oc = g.kpatch;
  g.c_rows = c.cond_type == DFOT_COND_LABEL ? c.num_classes + (c.cond_dropout ? 1 : 0) : 0;
  g.diffm = c.variant == 1, g.facmat = c.variant == 1 || c.variant == 3, g.fac = c.variant == 2;
  return g;
}

// what a tensor is, so that an engine binds storage without reading the name
enum DitKind {
  DIT_FZ_FREQS, DIT_FZ_PHASES,                                                     // FourierEmbedding's persistent buffers
  DIT_T_W1, DIT_T_B1, DIT_T_W2, DIT_T_B2,                                          // noise-level embedding MLP
  DIT_C_W1, DIT_C_B1, DIT_C_W2, DIT_C_B2, DIT_C_TABLE,                             // external condition: action MLP / label table
  DIT_PE_W, DIT_PE_B, DIT_DIFF,                                                    // patch embedding, diff_embedder (variant 1)
  DIT_MOD1_W, DIT_MOD1_B, DIT_QKV_W, DIT_QKV_B, DIT_PROJ_W, DIT_PROJ_B,            // DiTBlock: norm1, attn
  DIT_QKV_U, DIT_PROJ_U, DIT_QKV_V, DIT_PROJ_V, DIT_QKV_BIAS, DIT_PROJ_BIAS,       // MatrixDiTBlock: attn factors, stored (in, out)
  DIT_MOD2_W, DIT_MOD2_B, DIT_FC1_W, DIT_FC1_B, DIT_FC2_W, DIT_FC2_B,              // norm2 + mlp of either block
  DIT_FMOD_W, DIT_FMOD_B, DIT_FIN_W, DIT_FIN_B                                     // final layer
};

struct DitTensor {
  std::string name;
  std::vector<int64_t> shape;
  DitKind kind;
  int block = -1;         // index in dit_base.blocks / dit_base.temporal_blocks (-1: outside the blocks)
  bool temporal = false;  // member of dit_base.temporal_blocks
  long col = -1;          // modulation Linears: first column of the modulation table (= first row of the stacked weight)
  bool buffer = false;    // persistent buffer, not a parameter: the inference engine loads it, the trainer keeps it out of the flat buffers
  long offset = -1;       // parameters, after dit_flat_layout: start in the flat parameter / gradient buffers
  long numel() const {
    long n = 1;
    for (int64_t v : shape) n *= v;
    return n;
  }
};

// every tensor of the reference module, in its state_dict() order
inline std::vector<DitTensor> dit_inventory(const DitCfg& c) {
  const DitGeom g = dit_grid(c);
  const int hd = c.hidden_size, E = c.embed_col_dim, P = g.P, ps = c.patch_size;
  std::vector<DitTensor> inv;
  int block = -1;
  bool temporal = false;
  long col = 0;
  auto add = [&](const std::string& name, DitKind kind, std::vector<int64_t> shape, long at = -1) {
    DitTensor t;
    t.name = name, t.shape = std::move(shape), t.kind = kind, t.block = block, t.temporal = temporal, t.col = at;
    t.buffer = kind == DIT_FZ_FREQS || kind == DIT_FZ_PHASES;
    inv.push_back(std::move(t));
  };
  auto linear = [&](const std::string& pre, DitKind weight, DitKind bias, int out, int in) {
    add(pre + ".weight", weight, {out, in});
    add(pre + ".bias", bias, {out});
  };
  auto modulation = [&](const std::string& norm, DitKind weight, DitKind bias, int out) {  // AdaLN: Sequential(SiLU, Linear(hidden, out))
    add(norm + ".modulation.1.weight", weight, {out, hd}, col);
    add(norm + ".modulation.1.bias", bias, {out}, col);
    col += out;
  };
  auto mlp = [&](const std::string& pre, int width) {  // norm2 + Mlp: the same six tensors in every kind of block (none at width 0)
    if (!width) return;
    modulation(pre + ".norm2", DIT_MOD2_W, DIT_MOD2_B, 3 * hd);
    linear(pre + ".mlp.fc1", DIT_FC1_W, DIT_FC1_B, width, hd);
    linear(pre + ".mlp.fc2", DIT_FC2_W, DIT_FC2_B, hd, width);
  };
  auto dit_block = [&](const std::string& pre, int width) {
    modulation(pre + ".norm1", DIT_MOD1_W, DIT_MOD1_B, 3 * hd);
    linear(pre + ".attn.qkv", DIT_QKV_W, DIT_QKV_B, 3 * hd, hd);
    linear(pre + ".attn.proj", DIT_PROJ_W, DIT_PROJ_B, hd, hd);
    mlp(pre, width);
  };

  if (c.fourier_noise) {  // state_dict lists noise_level_pos_embedding.timesteps before .embedding
    add("noise_level_pos_embedding.timesteps.freqs", DIT_FZ_FREQS, {c.noise_dim});
    add("noise_level_pos_embedding.timesteps.phases", DIT_FZ_PHASES, {c.noise_dim});
  }
  linear("noise_level_pos_embedding.embedding.linear_1", DIT_T_W1, DIT_T_B1, hd, c.noise_dim);
  linear("noise_level_pos_embedding.embedding.linear_2", DIT_T_W2, DIT_T_B2, hd, hd);
  // BaseBackbone builds external_cond_embedding right after the noise-level embedding (base_backbone.py:35-62)
  if (c.cond_type == DFOT_COND_ACTION) {
    const std::string ce = std::string("external_cond_embedding") + (c.cond_dropout ? ".embedding" : "");
    linear(ce + ".linear_1", DIT_C_W1, DIT_C_B1, hd, c.cond_dim);
    linear(ce + ".linear_2", DIT_C_W2, DIT_C_B2, hd, hd);
  } else if (c.cond_type == DFOT_COND_LABEL) {
    add("external_cond_embedding.embedding_table.weight", DIT_C_TABLE, {g.c_rows, hd});
  }
  add("patch_embedder.proj.weight", DIT_PE_W, {hd, c.in_channels, ps, ps});
  add("patch_embedder.proj.bias", DIT_PE_B, {hd});
  if (g.diffm) add("diff_embedder.embedding_table.weight", DIT_DIFF, {2, hd});
  // all spatial blocks, then all temporal blocks: DiTBlocks (variant 2) or MatrixDiTBlocks (variants 1 and 3)
  for (block = 0; block < c.depth; ++block) dit_block("dit_base.blocks." + std::to_string(block), c.mlp_hidden);
  temporal = true;
  for (block = 0; block < (g.fac || g.facmat ? c.depth : 0); ++block) {
    const std::string pre = "dit_base.temporal_blocks." + std::to_string(block);
    if (g.fac) {
      dit_block(pre, c.temporal_mlp_hidden);
      continue;
    }
    modulation(pre + ".norm1", DIT_MOD1_W, DIT_MOD1_B, 3 * hd);
    add(pre + ".attn.qkv_u", DIT_QKV_U, {P, E});
    add(pre + ".attn.proj_u", DIT_PROJ_U, {E, P});
    add(pre + ".attn.qkv_v", DIT_QKV_V, {hd, 3 * hd});
    add(pre + ".attn.proj_v", DIT_PROJ_V, {hd, hd});
    if (c.use_bias) {
      add(pre + ".attn.qkv_bias", DIT_QKV_BIAS, {E, 3 * hd});
      add(pre + ".attn.proj_bias", DIT_PROJ_BIAS, {P, hd});
    }
    mlp(pre, c.temporal_mlp_hidden);
  }
  block = -1, temporal = false;
  modulation("dit_base.final_layer.norm_final", DIT_FMOD_W, DIT_FMOD_B, 2 * hd);
  linear("dit_base.final_layer.linear", DIT_FIN_W, DIT_FIN_B, g.oc, hd);
  return inv;
}

// the whole geometry: the final layer's modulation is the last one the inventory lists, and the table ends with it
inline DitGeom dit_geometry(const DitCfg& c) {
  DitGeom g = dit_grid(c);
  for (const DitTensor& t : dit_inventory(c))
    if (t.kind == DIT_FMOD_W) g.mod_final = t.col, g.ldt = t.col + t.shape[0];
  return g;
}

// The trainer's flat parameter / gradient buffers: the parameters in inventory order, every tensor 16-byte aligned (its element count
// rounded up to a multiple of 4).  Sets DitTensor::offset, returns the buffers' length in floats.
inline long dit_flat_layout(std::vector<DitTensor>& inv) {
  long total = 0;
  for (DitTensor& t : inv) {
    if (t.buffer) continue;
    t.offset = total;
    total += (t.numel() + 3) / 4 * 4;
  }
  return total;
}

// ---- host-computed tables -------------------------------------------------------------------------------------------
// get_timestep_embedding's frequencies [noise_dim / 2]: exp(-ln(10000) i / half), in float64
inline std::vector<float> dit_timestep_freqs(const DitCfg& c) {
  const int half = c.noise_dim / 2;
  std::vector<float> f(half);
  for (int i = 0; i < half; ++i) f[i] = (float)std::exp(-std::log(10000.0) * (double)i / (double)half);
  return f;
}

// out[0..2n) = [sin | cos] of pos * 10000^(-i/n), computed in float64 like numpy (get_1d_sincos_pos_embed_from_grid, dit_base.py:552-572)
inline void dit_sincos(int pos, int n, float* out) {
  for (int i = 0; i < n; ++i) {
    const double ang = (double)pos / std::pow(10000.0, (double)i / (double)n);
    out[i] = (float)std::sin(ang);
    out[n + i] = (float)std::cos(ang);
  }
}

// sinusoidal_2d table [P][hidden] (get_nd_sincos_pos_embed, dit_base.py:527-572): np.meshgrid's default "xy" indexing makes flattened
// entry m use position m % gh for the first half of the channels and m / gh for the second
inline std::vector<float> dit_sinusoidal_2d(const DitCfg& c, const DitGeom& g) {
  const int hd = c.hidden_size, half = hd / 2, quarter = half / 2;
  std::vector<float> pe((size_t)g.P * hd);
  for (int m = 0; m < g.P; ++m) {
    const int pos[2] = {m % g.gh, m / g.gh};
    for (int a = 0; a < 2; ++a) dit_sincos(pos[a], quarter, &pe[(size_t)m * hd + a * half]);
  }
  return pe;
}

// temporal table [max_tokens][hidden] of variant 2 (SinusoidalPositionalEmbedding of the 1-D shape (max_tokens,), dit_base.py:268-271)
inline std::vector<float> dit_sinusoidal_1d(const DitCfg& c) {
  const int hd = c.hidden_size;
  std::vector<float> te((size_t)c.max_tokens * hd);
  for (int t = 0; t < c.max_tokens; ++t) dit_sincos(t, hd / 2, &te[(size_t)t * hd]);
  return te;
}

// RotaryEmbedding1D(dim = embed_row_dim / num_row_heads, seq_len = max_tokens) of variant 3 (dit_base.py:297-306; embeddings.py:193-202):
// (cos, sin) [max_tokens][dim/2][2] of angle = frame * theta^(-2i/dim) for the pair i of every matrix row, in float64
inline std::vector<float> dit_rope_1d(const DitCfg& c) {
  const int dim = c.hidden_size / c.num_row_heads, pairs = dim / 2;
  std::vector<float> cs((size_t)c.max_tokens * pairs * 2);
  for (int t = 0; t < c.max_tokens; ++t)
    for (int i = 0; i < pairs; ++i) {
      const double ang = (double)t * std::pow((double)c.rope_theta, -2.0 * (double)i / (double)dim);
      cs[((size_t)t * pairs + i) * 2 + 0] = (float)std::cos(ang);
      cs[((size_t)t * pairs + i) * 2 + 1] = (float)std::sin(ang);
    }
  return cs;
}

// RoPE-3D (cos, sin) table [max_tokens * P][d/2][2] of variant 0, in fp32 as the reference; axis split of the head dim as
// RotaryEmbedding3D (embeddings.py:251-277)
inline std::vector<float> dit_rope_3d(const DitCfg& c, const DitGeom& g) {
  const int half = g.d / 2, q = half / 3, rem = half % 3;
  int parts[3] = {q, q, q};
  if (rem == 1) parts[0] = q + 1;
  if (rem == 2) parts[1] = parts[2] = q + 1;
  const int n = c.max_tokens * g.P;
  std::vector<float> cs((size_t)n * half * 2);
  for (int tok = 0; tok < n; ++tok) {
    const int pos[3] = {tok / g.P, (tok / g.gw) % g.gh, tok % g.gw};
    int pair = 0;
    for (int ax = 0; ax < 3; ++ax) {
      const int dim = 2 * parts[ax];
      for (int j = 0; j < parts[ax]; ++j, ++pair) {
        const float inv = 1.0f / powf(c.rope_theta, (float)(2 * j) / (float)dim);
        const float ang = (float)pos[ax] * inv;
        cs[((size_t)tok * half + pair) * 2 + 0] = cosf(ang);
        cs[((size_t)tok * half + pair) * 2 + 1] = sinf(ang);
      }
    }
  }
  return cs;
}

}  // namespace dfot
