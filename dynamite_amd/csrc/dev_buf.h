// Device allocation that frees itself (alloc / upload / release: mat.cpp -- the only HIP calls behind the host tables of
// mat.h and sc3.h, so that their builders compile and run without a device).
#pragma once

#include <cstddef>
#include <vector>

namespace dnm {

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  int alloc(size_t nbytes);
  int upload(const void *host, size_t nbytes);
  template <class T>
  int upload(const std::vector<T> &v) { return upload(v.data(), v.size() * sizeof(T)); }
  template <class T>
  const T *as() const { return static_cast<const T *>(p); }
  void release();
};

}  // namespace dnm
