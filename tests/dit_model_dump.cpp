// Prints the host-side description of a DiT model (csrc/dit_model.h) for tests/test_dit_model_host.py: no GPU, no HIP.
//   dit_model_dump <outdir> field=value ...      fields of dfot_dit_config, and fourier_noise; unset fields are 0
// stdout: "# key=value ..." (the geometry and the flat buffers' length), then one line per tensor of the inventory:
//   name shape... k<kind> block temporal buffer col offset
// <outdir>: freqs.f32, pos2d.f32, tpos.f32, rope3d.f32 and (num_row_heads > 0) rope1d.f32, raw fp32
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dit_model.h"

static bool set_field(DitCfg& c, const char* key, const char* value) {
#define FIELD(name)                                 \
  if (!strcmp(key, #name)) {                        \
    c.name = (decltype(c.name))strtod(value, nullptr); \
    return true;                                    \
  }
  FIELD(hidden_size) FIELD(depth) FIELD(num_heads) FIELD(patch_size) FIELD(in_channels) FIELD(height) FIELD(width) FIELD(max_tokens)
  FIELD(mlp_hidden) FIELD(noise_dim) FIELD(timesteps) FIELD(rope_theta) FIELD(eps) FIELD(variant) FIELD(embed_col_dim)
  FIELD(num_col_heads) FIELD(num_row_heads) FIELD(temporal_mlp_hidden) FIELD(use_bias) FIELD(cond_type) FIELD(cond_dim)
  FIELD(num_classes) FIELD(cond_dropout) FIELD(use_temporal_rope) FIELD(fourier_noise)
#undef FIELD
  return false;
}

static bool write_table(const std::string& dir, const char* name, const std::vector<float>& v) {
  FILE* f = fopen((dir + "/" + name).c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <outdir> field=value ...\n", argv[0]);
    return 2;
  }
  DitCfg c = dit_cfg(dfot_dit_config{});
  for (int i = 2; i < argc; ++i) {
    std::string arg = argv[i];
    const size_t eq = arg.find('=');
    if (eq == std::string::npos || !set_field(c, arg.substr(0, eq).c_str(), arg.c_str() + eq + 1)) {
      fprintf(stderr, "unknown argument '%s'\n", argv[i]);
      return 2;
    }
  }
  const dfot::DitGeom g = dfot::dit_geometry(c);
  std::vector<dfot::DitTensor> inv = dfot::dit_inventory(c);
  const long total = dfot::dit_flat_layout(inv);
  printf("# gh=%d gw=%d P=%d d=%d dstride=%d kpatch=%d oc=%d c_rows=%d ldt=%ld mod_final=%ld diffm=%d facmat=%d fac=%d total=%ld\n", g.gh, g.gw,
         g.P, g.d, g.dstride, g.kpatch, g.oc, g.c_rows, g.ldt, g.mod_final, (int)g.diffm, (int)g.facmat, (int)g.fac, total);
  for (const dfot::DitTensor& t : inv) {
    printf("%s", t.name.c_str());
    for (int64_t v : t.shape) printf(" %lld", (long long)v);
    printf(" k%d %d %d %d %ld %ld\n", (int)t.kind, t.block, (int)t.temporal, (int)t.buffer, t.col, t.offset);
  }
  const std::string dir = argv[1];
  bool ok = write_table(dir, "freqs.f32", dfot::dit_timestep_freqs(c)) && write_table(dir, "pos2d.f32", dfot::dit_sinusoidal_2d(c, g)) &&
            write_table(dir, "tpos.f32", dfot::dit_sinusoidal_1d(c)) && write_table(dir, "rope3d.f32", dfot::dit_rope_3d(c, g));
  if (c.num_row_heads > 0) ok = ok && write_table(dir, "rope1d.f32", dfot::dit_rope_1d(c));
  if (!ok) fprintf(stderr, "cannot write the tables to '%s'\n", dir.c_str());
  return ok ? 0 : 1;
}
