// Internal: an owned device allocation, and the two ways the handle uploads a
// table that launches captured into a graph go on reading:
//   in place  one allocation of the largest size, made once, so the address a
//             captured launch holds stays valid whatever is uploaded later;
//   replace   the new table is allocated and filled first, the caller drains
//             the device and re-points the kernels, and only then does the
//             move-assignment free the old table; a failure on the way frees
//             the new table and leaves the old one where it was.
// A failed call leaves "<call>: <HIP's text>" in `err`, `call` as given.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <string>

struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      ptr = o.ptr, bytes = o.bytes;
      o.ptr = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr, bytes = 0;
  }
  hipError_t alloc(size_t n) {   // of an empty buffer
    if (ptr) return hipErrorInvalidValue;
    const hipError_t e = hipMalloc(&ptr, n);
    if (e != hipSuccess) ptr = nullptr;
    bytes = ptr ? n : 0;
    return e;
  }
};

inline hipError_t hip_said(std::string& err, const char* call, hipError_t e) {
  if (e != hipSuccess) err = std::string(call) + ": " + hipGetErrorString(e);
  return e;
}

struct UploadCalls {
  const char *alloc, *sync, *copy;
};

// In place: allocates `capacity` bytes if `b` is empty, drains the device, then
// copies `bytes` <= capacity.  Nothing to copy: the drain alone, no allocation.
inline hipError_t upload_in_place(DevBuf& b, size_t capacity, const void* src, size_t bytes,
                                  const UploadCalls& calls, std::string& err) {
  if (bytes > (b.ptr ? b.bytes : capacity)) return hip_said(err, calls.copy, hipErrorInvalidValue);
  hipError_t e = hipSuccess;
  if (bytes && !b.ptr) e = hip_said(err, calls.alloc, b.alloc(capacity));
  if (e == hipSuccess) e = hip_said(err, calls.sync, hipDeviceSynchronize());
  if (e == hipSuccess && bytes)
    e = hip_said(err, calls.copy, hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice));
  return e;
}

// Replace, first half: `fresh` (empty) takes a new allocation holding `bytes`
// of `src`, or stays empty.  The second half is `table = std::move(fresh)`.
inline hipError_t upload_new(DevBuf& fresh, const void* src, size_t bytes, const char* alloc_call,
                             const char* copy_call, std::string& err) {
  hipError_t e = hip_said(err, alloc_call, fresh.alloc(bytes));
  if (e != hipSuccess) return e;
  e = hip_said(err, copy_call, hipMemcpy(fresh.ptr, src, bytes, hipMemcpyHostToDevice));
  if (e != hipSuccess) fresh.reset();
  return e;
}
