// A set of HIP events that lives as long as its scope (the tpnet_time_* entry points): created together, destroyed together on
// every way out.  Needs the runtime's C API only, so that it can be built and tested without a device compiler.
#pragma once
#include <hip/hip_runtime_api.h>
#include <vector>

namespace tpnet {

class EventSet {
    std::vector<hipEvent_t> ev_;          // created so far: what the destructor destroys
    hipError_t err_ = hipSuccess;
  public:
    explicit EventSet(size_t n) {
        ev_.reserve(n);
        for (size_t i = 0; i < n && err_ == hipSuccess; ++i) {
            hipEvent_t e = nullptr;
            err_ = hipEventCreate(&e);
            if (err_ == hipSuccess) ev_.push_back(e);
        }
    }
    ~EventSet() { for (hipEvent_t e : ev_) (void)hipEventDestroy(e); }
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    hipError_t error() const { return err_; }        // hipSuccess: all n events exist
    hipEvent_t operator[](size_t i) const { return ev_[i]; }
    hipEvent_t* data() { return ev_.data(); }
};

}  // namespace tpnet
