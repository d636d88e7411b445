// fdcn_host_call.h -- the staging every host-array entry point of libfdcn
// shares, kept free of HIP calls so it runs on the CPU under the sanitizers
// (tools/sanitize/host_call_driver.cpp), as fdcn_session_book.h does:
//   HostCall        one call's device arrays as 256-byte-aligned regions of
//                   one stream-ordered block: copies in, the caller's launch,
//                   copies out, free, synchronise -- the threading contract of
//                   fdcn.h (own stream, pooled block, no device-wide wait)
//   with_workspace  the scratch of a `_dev` entry point: the caller's buffer,
//                   or a stream-ordered one released on every path out
// Backend (a template parameter: HipCall of fdcn_shared.h in the library,
// malloc / memcpy in the driver) supplies
//   using Stream;
//   static int open(Stream*);              device check + the thread's stream;
//                                          reports its own failure
//   static const char* alloc(void**, size_t, Stream);     nullptr, or the
//   static const char* release(void*, Stream);            failure's text
//   static const char* copy_in(void* dev, const void* host, size_t, Stream);
//   static const char* copy_out(void* host, const void* dev, size_t, Stream);
//   static const char* sync(Stream);
//   static int fail(int code, const char* msg);           records msg, returns code
// Failures read "<entry>: <step> failed: <text>"; the first one of a call is
// the one its caller gets.
#ifndef FDCN_HOST_CALL_H
#define FDCN_HOST_CALL_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fdcn.h"
#include "fdcn_session_book.h"

namespace fdcn_call {

template <class B>
int step_failed(int code, const char* entry, const char* step, const char* text) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s failed: %s", entry, step, text);
  return B::fail(code, msg);
}

template <class B>
class HostCall {
 public:
  explicit HostCall(const char* entry) : entry_(entry) {}
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;

  // device check, then the calling thread's stream
  int open() { return B::open(&stream_); }

  // Regions, declared in the order they lie in the block; the number each
  // returns is what dev() takes inside the launch.  An array the caller left
  // out (host == nullptr) takes no room and its device pointer is null --
  // unless `reserve` bytes are asked for: then the region exists whatever
  // `host` is, and `bytes` (possibly 0) of it are copied in.
  int in(const void* host, size_t bytes, size_t reserve = 0) {
    return add(host, nullptr, bytes, reserve > bytes ? reserve : bytes, host || reserve);
  }
  int out(void* host, size_t bytes) { return add(nullptr, host, bytes, bytes, host != nullptr); }
  int scratch(size_t bytes) { return add(nullptr, nullptr, 0, bytes, true); }

  template <class T>
  T* dev(int region) const {
    const Region& r = regions_[region];
    return r.present ? reinterpret_cast<T*>(block_ + r.offset) : nullptr;
  }
  size_t offset(int region) const { return regions_[region].offset; }
  size_t block_bytes() const { return layout_.size; }

  // allocate; copies in; launch(stream) -> FDCN_OK or the code of a failure
  // it has reported; copies out if all of that succeeded; free; synchronise.
  // The host outputs are written only by the copies out, and may be read
  // once run() has returned.
  template <class Launch>
  int run(Launch launch) {
    if (n_ > kMaxRegions) return B::fail(FDCN_EINVAL, "host call: too many regions");
    void* p = nullptr;
    const char* e = B::alloc(&p, layout_.size, stream_);
    if (e) return step_failed<B>(FDCN_ENOMEM, entry_, "allocation", e);
    block_ = static_cast<char*>(p);
    int rc = FDCN_OK;
    for (int i = 0; i < n_ && rc == FDCN_OK; ++i) {
      const Region& r = regions_[i];
      if (r.present && r.host_in && r.bytes &&
          (e = B::copy_in(block_ + r.offset, r.host_in, r.bytes, stream_)))
        rc = step_failed<B>(FDCN_EHIP, entry_, "copy to the device", e);
    }
    if (rc == FDCN_OK) rc = launch(stream_);
    for (int i = 0; i < n_ && rc == FDCN_OK; ++i) {
      const Region& r = regions_[i];
      if (r.present && r.host_out && r.bytes &&
          (e = B::copy_out(r.host_out, block_ + r.offset, r.bytes, stream_)))
        rc = step_failed<B>(FDCN_EHIP, entry_, "copy from the device", e);
    }
    e = B::release(block_, stream_);
    block_ = nullptr;
    if (e && rc == FDCN_OK) rc = step_failed<B>(FDCN_EHIP, entry_, "free", e);
    e = B::sync(stream_);
    if (e && rc == FDCN_OK) rc = step_failed<B>(FDCN_EHIP, entry_, "kernel / copies", e);
    return rc;
  }

 private:
  static constexpr int kMaxRegions = 12;
  struct Region {
    const void* host_in;
    void* host_out;
    size_t bytes, offset;
    bool present;
  };

  int add(const void* host_in, void* host_out, size_t bytes, size_t room, bool present) {
    if (n_ >= kMaxRegions) return n_ = kMaxRegions + 1, 0;  // run() refuses
    regions_[n_] = {host_in, host_out, bytes, present ? layout_.add(room) : 0, present};
    return n_++;
  }

  const char* entry_;
  typename B::Stream stream_{};
  fdcn_book::Layout layout_;
  Region regions_[kMaxRegions];
  int n_ = 0;
  char* block_ = nullptr;
};

// The scratch of a `_dev` launch on `stream`: `caller` if it holds `need`
// bytes (a smaller one is FDCN_EINVAL, "<entry>: workspace of .. B is smaller
// than the .. B <tail>"), or, for a null `caller`, a stream-ordered block
// that is released after launch(workspace) whatever it returned.  Nothing
// here waits for the device.
template <class B, class Launch>
int with_workspace(const char* entry, const char* tail, void* caller, int64_t caller_bytes,
                   int64_t need, typename B::Stream stream, Launch launch) {
  if (caller) {
    if (caller_bytes >= need) return launch(caller);
    char msg[256];
    snprintf(msg, sizeof msg, "%s: workspace of %lld B is smaller than the %lld B %s", entry,
             (long long)caller_bytes, (long long)need, tail);
    return B::fail(FDCN_EINVAL, msg);
  }
  void* own = nullptr;
  const char* e = B::alloc(&own, (size_t)need, stream);
  if (e) return step_failed<B>(FDCN_ENOMEM, entry, "workspace allocation", e);
  int rc = launch(own);
  e = B::release(own, stream);
  if (e && rc == FDCN_OK) rc = step_failed<B>(FDCN_EHIP, entry, "workspace free", e);
  return rc;
}

}  // namespace fdcn_call

#endif  // FDCN_HOST_CALL_H
