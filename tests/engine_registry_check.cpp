// Host check of csrc/engine_registry.h, the parameter registry of the inference engines: compiled with the host compiler alone (no HIP
// header) by tests/test_engine_registry_host.py.  The loaders only record their calls; the stream is an int.  Prints "ok" and exits 0,
// or names the first expectation that failed and exits 1.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "engine_registry.h"

static char g_err[512] = "";
namespace dfot {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace dfot

static int g_failed = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
      g_failed = 1;                                                  \
    }                                                                \
  } while (0)
#define EXPECT_ERR(expr, code, text) \
  do {                               \
    g_err[0] = 0;                    \
    EXPECT((expr) == (code));        \
    EXPECT(!strcmp(g_err, text));    \
  } while (0)

struct Call {
  std::string name;
  const float* data;
  int stream;
};

static void check(const std::string& prefix) {
  using Registry = dfot::ParamRegistry<int>;
  Registry reg(prefix);
  std::vector<Call> calls;
  int fail_with = 0;  // what the loader of "b.bias" returns
  const std::vector<std::pair<std::string, std::vector<int64_t>>> layout = {
      {"z.weight", {2, 3, 4, 5}}, {"a.weight", {7, 3}}, {"b.bias", {6}}, {"scalar", {}}};
  for (const auto& [name, shape] : layout) {
    const bool may_fail = name == "b.bias";
    reg.add(name, shape, [&calls, &fail_with, may_fail, n = name](const float* src, int stream) {
      calls.push_back(Call{n, src, stream});
      return may_fail ? fail_with : 0;
    });
  }
  const std::string p = prefix;

  // registration order is enumeration order (not the name order of the index); shapes come back as given, up to 4 dimensions
  EXPECT(reg.count() == 4);
  for (int i = 0; i < 4; ++i) {
    int64_t shape[4] = {-1, -1, -1, -1};
    int ndim = -1;
    EXPECT(reg.name(i) && layout[i].first == reg.name(i));
    EXPECT(reg.shape(i, shape, &ndim) == DFOT_OK && ndim == (int)layout[i].second.size());
    for (int k = 0; k < 4; ++k) EXPECT(shape[k] == (k < ndim ? layout[i].second[k] : -1));
  }
  EXPECT(reg.name(-1) == nullptr && reg.name(4) == nullptr);
  int64_t shape[4];
  int ndim = 0;
  EXPECT_ERR(reg.shape(4, shape, &ndim), DFOT_ERR_ARG, (p + "param_shape: bad argument").c_str());
  EXPECT_ERR(reg.shape(-1, shape, &ndim), DFOT_ERR_ARG, (p + "param_shape: bad argument").c_str());
  EXPECT_ERR(reg.shape(0, nullptr, &ndim), DFOT_ERR_ARG, (p + "param_shape: bad argument").c_str());
  EXPECT_ERR(reg.shape(0, shape, nullptr), DFOT_ERR_ARG, (p + "param_shape: bad argument").c_str());

  // nothing loaded: the first missing entry is the first registered one
  EXPECT(reg.first_missing() && !strcmp(reg.first_missing(), "z.weight"));
  EXPECT_ERR(reg.require_all_loaded(), DFOT_ERR_STATE, (p + "finalize: missing key 'z.weight'").c_str());

  const float data[1] = {0.f};
  const int64_t s_a[2] = {7, 3}, s_a_extent[2] = {7, 4}, s_z[4] = {2, 3, 4, 5}, s_b[1] = {6};
  // refusals: none of them runs a loader or marks an entry
  EXPECT_ERR(reg.load(nullptr, data, s_a, 2, 1), DFOT_ERR_ARG, (p + "load_weight: null argument").c_str());
  EXPECT_ERR(reg.load("a.weight", nullptr, s_a, 2, 1), DFOT_ERR_ARG, (p + "load_weight: null argument").c_str());
  EXPECT_ERR(reg.load("a.weight", data, nullptr, 2, 1), DFOT_ERR_ARG, (p + "load_weight: null argument").c_str());
  EXPECT_ERR(reg.load("a.weights", data, s_a, 2, 1), DFOT_ERR_NAME, (p + "load_weight: unexpected key 'a.weights'").c_str());
  EXPECT_ERR(reg.load("a.weight", data, s_a, 1, 1), DFOT_ERR_SHAPE, (p + "load_weight: size mismatch for 'a.weight'").c_str());      // rank
  EXPECT_ERR(reg.load("a.weight", data, s_z, 4, 1), DFOT_ERR_SHAPE, (p + "load_weight: size mismatch for 'a.weight'").c_str());      // rank
  EXPECT_ERR(reg.load("a.weight", data, s_a_extent, 2, 1), DFOT_ERR_SHAPE, (p + "load_weight: size mismatch for 'a.weight'").c_str());  // extent
  EXPECT_ERR(reg.load("scalar", data, s_a, 1, 1), DFOT_ERR_SHAPE, (p + "load_weight: size mismatch for 'scalar'").c_str());
  EXPECT(calls.empty() && !strcmp(reg.first_missing(), "z.weight"));

  // a load runs the loader with the data and the stream it was given, and marks the entry
  EXPECT(reg.load("a.weight", data, s_a, 2, 11) == DFOT_OK);
  EXPECT(calls.size() == 1 && calls[0].name == "a.weight" && calls[0].data == data && calls[0].stream == 11);
  EXPECT(!strcmp(reg.first_missing(), "z.weight"));  // still the earliest in registration order
  EXPECT(reg.load("z.weight", data, s_z, 4, 12) == DFOT_OK);
  EXPECT(!strcmp(reg.first_missing(), "b.bias"));

  // a loader's failure code is passed through and leaves the entry unloaded
  fail_with = DFOT_ERR_HIP;
  EXPECT(reg.load("b.bias", data, s_b, 1, 13) == DFOT_ERR_HIP);
  EXPECT(calls.size() == 3 && calls[2].name == "b.bias" && !strcmp(reg.first_missing(), "b.bias"));
  fail_with = 0;
  EXPECT(reg.load("b.bias", data, s_b, 1, 13) == DFOT_OK);
  EXPECT_ERR(reg.require_all_loaded(), DFOT_ERR_STATE, (p + "finalize: missing key 'scalar'").c_str());
  EXPECT(reg.load("scalar", data, s_a, 0, 14) == DFOT_OK);  // rank 0: the shape pointer is not read
  EXPECT(reg.first_missing() == nullptr && reg.require_all_loaded() == DFOT_OK);

  // loading the same name twice runs the loader twice
  const size_t before = calls.size();
  EXPECT(reg.load("a.weight", data, s_a, 2, 15) == DFOT_OK && reg.load("a.weight", data, s_a, 2, 16) == DFOT_OK);
  EXPECT(calls.size() == before + 2 && calls[before].stream == 15 && calls[before + 1].stream == 16);
  EXPECT(reg.first_missing() == nullptr);
}

int main() {
  check("");        // dit, uvit
  check("dit1d ");  // dit1d
  dfot::ParamRegistry<int> empty;
  EXPECT(empty.count() == 0 && empty.name(0) == nullptr && empty.first_missing() == nullptr && empty.require_all_loaded() == DFOT_OK);
  if (!g_failed) printf("ok\n");
  return g_failed;
}
