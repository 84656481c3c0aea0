// The state-dict side of an inference engine (dit.hip, uvit.hip, dit1d.hip): the named parameters an engine registers while it
// builds, in the reference module's state_dict order, each with the loader that packs it into the engine's own storage.  The five
// entry points every engine exports (num_params, param_name, param_shape, load_weight and the "missing key" check of finalize) are
// these operations.  Host C++17 only (no HIP header): Stream is the engine's stream type, set_error the library's (common.h).
#pragma once
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "dfot_hip.h"

namespace dfot {

void set_error(const char* fmt, ...);

template <typename Stream>
class ParamRegistry {
 public:
  using Loader = std::function<int(const float*, Stream)>;

  // prefix: what the engine's messages start with ("" for dit / uvit, "dit1d " for dit1d)
  explicit ParamRegistry(std::string prefix = "") : prefix_(std::move(prefix)) {}

  void add(const std::string& name, std::vector<int64_t> shape, Loader load) {
    index_[name] = (int)params_.size();
    params_.push_back(Param{name, std::move(shape), std::move(load), false});
  }

  int count() const { return (int)params_.size(); }
  const char* name(int i) const { return i >= 0 && i < count() ? params_[i].name.c_str() : nullptr; }
  int shape(int i, int64_t shape[4], int* ndim) const {
    if (!shape || !ndim || i < 0 || i >= count()) return fail(DFOT_ERR_ARG, "param_shape: bad argument");
    *ndim = (int)params_[i].shape.size();
    for (int k = 0; k < *ndim; ++k) shape[k] = params_[i].shape[k];
    return DFOT_OK;
  }

  // runs the loader of `name` on `data` (fp32, the registered shape) and marks the entry loaded; a loader's failure code is passed on
  int load(const char* name, const float* data, const int64_t* shape, int ndim, Stream stream) {
    if (!name || !data || !shape) return fail(DFOT_ERR_ARG, "load_weight: null argument");
    auto it = index_.find(name);
    if (it == index_.end()) return fail(DFOT_ERR_NAME, "load_weight: unexpected key", name);
    Param& p = params_[it->second];
    bool same = (int)p.shape.size() == ndim;
    for (int k = 0; same && k < ndim; ++k) same = p.shape[k] == shape[k];
    if (!same) return fail(DFOT_ERR_SHAPE, "load_weight: size mismatch for", name);
    int rc = p.load(data, stream);
    if (rc) return rc;
    p.loaded = true;
    return DFOT_OK;
  }

  // the first entry, in registration order, that no load() has filled; nullptr once all are
  const char* first_missing() const {
    for (const Param& p : params_)
      if (!p.loaded) return p.name.c_str();
    return nullptr;
  }
  // finalize's check: DFOT_ERR_STATE naming first_missing()
  int require_all_loaded() const {
    const char* missing = first_missing();
    return missing ? fail(DFOT_ERR_STATE, "finalize: missing key", missing) : DFOT_OK;
  }

 private:
  struct Param {
    std::string name;
    std::vector<int64_t> shape;
    Loader load;
    bool loaded = false;
  };

  int fail(int code, const char* what, const char* key = nullptr) const {
    if (key) set_error("%s%s '%s'", prefix_.c_str(), what, key);
    else set_error("%s%s", prefix_.c_str(), what);
    return code;
  }

  std::string prefix_;
  std::vector<Param> params_;
  std::map<std::string, int> index_;
};

}  // namespace dfot
