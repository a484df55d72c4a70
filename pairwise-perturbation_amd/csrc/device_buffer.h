// device_buffer.h — the one owner of device memory in the engines and behind the C ABI: an allocation of an
// Ops that is freed when its owner goes away, however that happens. Descriptors (RTensor, PPOp, TensorDesc,
// Layout::ptr, ...) carry plain pointers INTO such buffers and never free anything.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "ops.h"

namespace ppals {

class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(Ops &ops, size_t bytes) : ops_(&ops), p_(ops.alloc(bytes)), bytes_(bytes) {}
  // takes over `p`, `bytes` long, that `ops` allocated (CpEngine::big_alloc, tensor_create); nullptr: empty
  DeviceBuffer(Ops &ops, void *p, size_t bytes) : ops_(&ops), p_(p), bytes_(p ? bytes : 0) {}
  // empty when the device is full (Ops::try_alloc)
  static DeviceBuffer try_alloc(Ops &ops, size_t bytes) { return DeviceBuffer(ops, ops.try_alloc(bytes), bytes); }
  DeviceBuffer(DeviceBuffer &&o) noexcept : ops_(o.ops_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  DeviceBuffer &operator=(DeviceBuffer &&o) {
    if (this != &o) {
      reset();
      ops_ = o.ops_, p_ = o.p_, bytes_ = o.bytes_;
      o.p_ = nullptr, o.bytes_ = 0;
    }
    return *this;
  }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  ~DeviceBuffer() {
    try {
      reset();
    } catch (...) {
    }
  }

  // frees now (Ops::free waits for what still reads the memory)
  void reset() {
    if (!p_) return;
    void *p = p_;
    p_ = nullptr, bytes_ = 0;
    ops_->free(p);
  }
  // gives the memory up to the caller, who frees it or hands it back to an owner (Ops::residual_slices)
  void *release() {
    void *p = p_;
    p_ = nullptr, bytes_ = 0;
    return p;
  }
  // grow-only, the contents are not kept: nothing when size() >= bytes; otherwise the old storage is freed
  // BEFORE the new one is taken (the device may not hold both), and an allocation that throws leaves the buffer
  // empty. True when the storage moved.
  bool reserve(Ops &ops, size_t bytes) {
    if (bytes_ >= bytes) return false;
    reset();
    *this = DeviceBuffer(ops, bytes);
    return true;
  }

  size_t size() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  void *get() const { return p_; }
  template <typename T>
  T *as() const {
    return static_cast<T *>(p_);
  }

 private:
  Ops *ops_ = nullptr;
  void *p_ = nullptr;
  size_t bytes_ = 0;
};

// One buffer of doubles per mode, with the table of their pointers that the ops take (FactorRef, Ops::normalize_ms,
// Ops::diff_norms, ...): t[i] and t.data() read as the vector of pointers this replaces.
class DeviceBufferTable {
 public:
  void resize(int n) {
    own_.resize((size_t)n);
    ptr_.assign((size_t)n, nullptr);
  }
  bool empty() const { return own_.empty(); }
  void alloc(Ops &ops, int i, size_t bytes) {
    own_[(size_t)i] = DeviceBuffer(ops, bytes);
    ptr_[(size_t)i] = own_[(size_t)i].as<double>();
  }
  // entry i changes places with entry i of `o` (TuckerEngine: the factor a deferred step replaces)
  void swap_entry(int i, DeviceBufferTable &o) {
    std::swap(own_[(size_t)i], o.own_[(size_t)i]);
    std::swap(ptr_[(size_t)i], o.ptr_[(size_t)i]);
  }
  double *operator[](int i) const { return ptr_[(size_t)i]; }
  double *const *data() const { return ptr_.data(); }

 private:
  std::vector<DeviceBuffer> own_;
  std::vector<double *> ptr_;
};

}  // namespace ppals
