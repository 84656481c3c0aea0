// The device side every inference engine handle (dfot_dit_s, dfot_uvit_s, dfot_dit1d_s) derives from: the parameter registry
// (engine_registry.h), the two allocation lists -- weights and derived tables live as long as the handle, the workspace until the next
// growing reserve -- and the loaders more than one engine registers.  A loader only one engine has stays in that engine and goes
// through params.add().
#pragma once
#include "common.h"
#include "engine_registry.h"
#include "kernels.h"

namespace dfot {

static inline int copy_f32(float* dst, const float* src, size_t n, hipStream_t s) {
  DFOT_CHECK_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return DFOT_OK;
}

struct EngineDevice {
  ParamRegistry<hipStream_t> params;
  std::vector<void*> owned, ws_owned;  // every hipMalloc'ed block
  size_t ws_bytes = 0;

  explicit EngineDevice(const char* prefix) : params(prefix) {}

  template <typename T>
  int alloc(T** out, size_t count, bool workspace = false) {
    void* p = nullptr;
    const size_t bytes = count * sizeof(T);
    DFOT_CHECK_HIP(hipMalloc(&p, bytes ? bytes : 16));
    (workspace ? ws_owned : owned).push_back(p);
    if (workspace) ws_bytes += bytes;
    *out = reinterpret_cast<T*>(p);
    return DFOT_OK;
  }
  void free_workspace() {
    for (void* p : ws_owned) (void)hipFree(p);
    ws_owned.clear();
    ws_bytes = 0;
  }
  void free_all() {
    for (void* p : owned) (void)hipFree(p);
    owned.clear();
    free_workspace();
  }

  static size_t numel(const std::vector<int64_t>& shape) {
    size_t n = 1;
    for (int64_t d : shape) n *= (size_t)d;
    return n;
  }
  // fp32 as given, at dst / in storage allocated here
  void add_slice(const std::string& name, std::vector<int64_t> shape, float* dst) {
    const size_t n = numel(shape);
    params.add(name, std::move(shape), [=](const float* src, hipStream_t s) { return copy_f32(dst, src, n, s); });
  }
  int add_f32(const std::string& name, std::vector<int64_t> shape, float** dst) {
    int rc = alloc(dst, numel(shape));
    if (!rc) add_slice(name, std::move(shape), *dst);
    return rc;
  }
  // Linear weight [rows][k] fp32 -> bf16 at dst (row stride k) / in storage allocated here
  void add_bf16(const std::string& name, int rows, int k, bf16* dst) {
    params.add(name, {rows, k}, [=](const float* src, hipStream_t s) { return launch_pack_rows(src, dst, nullptr, rows, k, k, k, 0, s); });
  }
  int add_linear(const std::string& name, int rows, int k, bf16** dst) {
    int rc = alloc(dst, (size_t)rows * k);
    if (!rc) add_bf16(name, rows, k, *dst);
    return rc;
  }
};

}  // namespace dfot
