// Workspace layouts, written once: a layout function walks a WsCursor through the slices of a `workspace` buffer.  On a null
// base it measures (dpm_*_workspace_bytes returns bytes()); on the caller's pointer it carves the very same slices.
#pragma once
#include <cstddef>
#include <cstdint>

constexpr size_t ws_align256(size_t v) { return (v + 255) & ~(size_t)255; }   // constexpr: the device-side accessors use it too

class WsCursor {   // host only
  public:
    // align_base: the first slice is the caller's pointer rounded up to 256 bytes, for which bytes() counts 256 bytes more
    explicit WsCursor(void *workspace, bool align_base = true)
        : base_(align_base ? ws_align256((uintptr_t)workspace) : (uintptr_t)workspace), off_(0), allowance_(align_base ? 256 : 0) {}
    template <class T> T *take(size_t n) {   // tight: n * sizeof(T) bytes at the current position
        T *at = (T *)(base_ + off_);
        off_ += n * sizeof(T);
        return at;
    }
    template <class T> T *take256(size_t n) {   // a slice that starts on, and is padded to, a multiple of 256 bytes from the base
        align256();
        T *at = take<T>(n);
        align256();
        return at;
    }
    void align256() { off_ = ws_align256(off_); }
    void skip(size_t bytes) { off_ += bytes; }   // a fixed gap a layout has always had: every use says which
    size_t bytes() const { return allowance_ + off_; }

  private:
    uintptr_t base_;
    size_t off_, allowance_;
};
