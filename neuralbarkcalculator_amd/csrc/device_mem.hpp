// Owners of the context's device memory (nbc_ctx.hpp): a growing buffer and a "borrowed or owned" array.  Both are templated
// on a memory policy, and no HIP header is included here, so tests/host/device_mem_test.cpp runs them on malloc.  A policy has
//   Error, ok()                              the error type and its "no error" value
//   Error allocate(void** p, size_t bytes)   *p is read only when ok() comes back
//   void  release(void* p)                   of a block allocate() gave; it is what waits for the work in flight
//   void  forget_error()                     after a refused allocate() that is tried again smaller
//   Error copy_in(void* dst, const void* host, size_t bytes)
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>

namespace nbc {

enum class Grow { kExact, kMargin };

// A block that only grows.  Move-only; released by the destructor.
template <class Mem>
class Buffer {
 public:
  using Error = typename Mem::Error;
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
    return *this;
  }
  ~Buffer() { reset(); }

  void* get() const { return p_; }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) Mem::release(p_); p_ = nullptr; cap_ = 0; }

  // Room for `need` bytes; nothing happens when they are there.  Otherwise the old block is released BEFORE the new one is
  // asked for (the peak stays at the larger of the two, and the release synchronises), and the contents are lost.  kMargin
  // asks for at least half as much again as it had -- sizes that rise one after the other then reallocate O(log) times --
  // and for exactly `need` when that is refused.  A refusal leaves the buffer empty and returns the policy's error.
  Error reserve(size_t need, Grow grow = Grow::kExact) {
    if (cap_ >= need) return Mem::ok();
    size_t want = grow == Grow::kMargin ? std::max(need, cap_ + cap_ / 2) : need;
    reset();
    Error e = Mem::allocate(&p_, want);
    if (e != Mem::ok() && want > need) {
      Mem::forget_error();
      want = need;
      e = Mem::allocate(&p_, want);
    }
    if (e != Mem::ok()) p_ = nullptr;
    else cap_ = want;
    return e;
  }

 private:
  void* p_ = nullptr;
  size_t cap_ = 0;
};

// `count` elements the context reads: the caller's (attach) or a block of its own (upload, adopt).  Move-only.
template <class T, class Mem>
class Array {
 public:
  using Error = typename Mem::Error;
  Array() = default;
  Array(Array&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)), owned_(std::move(o.owned_)) {}
  Array& operator=(Array&& o) noexcept {
    p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); owned_ = std::move(o.owned_);
    return *this;
  }

  const T* data() const { return p_; }
  size_t count() const { return n_; }

  // Points at the caller's memory and releases the block owned before -- unless `p` is that block, which stays owned.
  void attach(const T* p, size_t count) {
    if (owned_.get() != p) owned_.reset();
    p_ = p; n_ = count;
  }
  // Takes `block` over as the owned and attached one; the block owned before is released afterwards.
  void adopt(Buffer<Mem>&& block, size_t count) {
    p_ = block.template as<const T>(); n_ = count;
    owned_ = std::move(block);
  }
  // A new block with a copy of `count` host elements, adopted once both steps have succeeded (allocate first, release the old
  // block last: no moment without weights).  A failure leaves pointer, count and owned block as they were.
  Error upload(const T* host, size_t count) {
    Buffer<Mem> block;
    Error e = block.reserve(count * sizeof(T));
    if (e == Mem::ok()) e = Mem::copy_in(block.get(), host, count * sizeof(T));
    if (e == Mem::ok()) adopt(std::move(block), count);
    return e;
  }

 private:
  const T* p_ = nullptr;
  size_t n_ = 0;
  Buffer<Mem> owned_;
};

}  // namespace nbc
