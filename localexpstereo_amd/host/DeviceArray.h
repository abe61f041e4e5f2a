// DeviceArray.h -- the one owner of device memory above the C ABI (HipCostVolumeEnergy.h, PMStereo.h, les_host_demo.cpp), the host
// adapter's counterpart of DevBuf (csrc/les_hip_mem.h).  Plain C++ over include/localexp_hip.h: no HIP headers.
//
// The rule: every les_hip_malloc of the host adapter lives in a DeviceArray -- as a member (freed with its struct) or as a local (freed
// on every return path); what is handed across the ABI is still the caller's.  The steps of a staged call report to one Status.
#pragma once

#include <cstddef>
#include <cstdio>
#include <string>

#include "localexp_hip.h"

namespace les_host {

// The status of a sequence of C ABI calls: the first return code that is not LES_HIP_OK sticks, with the text les_hip_last_error() had
// right then (later calls overwrite that thread-local string), reported once on stderr as "<who>: <text>".  A DeviceArray's steps skip
// themselves once a step has failed; a library call is guarded with `if (st.ok())`.
struct Status {
    const char* who;
    int rc = LES_HIP_OK;
    std::string error;

    explicit Status(const char* who) : who(who) {}
    bool ok() const { return rc == LES_HIP_OK; }
    bool operator()(int step_rc)                           // records one step's return code -> ok()
    {
        if (ok() && step_rc != LES_HIP_OK) {
            rc = step_rc;
            error = les_hip_last_error();
            fprintf(stderr, "%s: %s\n", who, error.c_str());
        }
        return ok();
    }
};

// Move-only owner of n elements of T in a context's device memory; its steps report to the Status it was made with.
template <class T> class DeviceArray {
public:
    DeviceArray(les_hip_ctx* ctx, Status& st) : ctx_(ctx), st_(&st) {}
    DeviceArray(les_hip_ctx* ctx, Status& st, size_t n) : DeviceArray(ctx, st) { alloc(n); }                         // an output map
    DeviceArray(les_hip_ctx* ctx, Status& st, const T* host, size_t n) : DeviceArray(ctx, st) { upload(host, n); }   // an input map
    DeviceArray(DeviceArray&& o) noexcept : ctx_(o.ctx_), st_(o.st_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }      // (deletes the copies)
    ~DeviceArray() { reset(); }

    T* get() const { return p_; }
    size_t size() const { return n_; }
    void reset() { if (p_) les_hip_free(ctx_, p_); p_ = nullptr; n_ = 0; }
    // n elements (0: none, get() stays null -- an optional map that was not asked for); what the array held before is released first
    bool alloc(size_t n)
    {
        reset();
        if (n && st_->ok() && (*st_)(les_hip_malloc(ctx_, (void**)&p_, n * sizeof(T)))) n_ = n;
        return st_->ok();
    }
    // room for n elements: nothing happens when there is; the old contents are not kept
    bool grow(size_t n) { return n <= n_ ? st_->ok() : alloc(n); }
    // n elements from host memory, after grow(n); a null host pointer (an optional map that was not given) allocates nothing
    bool upload(const T* host, size_t n)
    {
        if (host && grow(n) && n) (*st_)(les_hip_memcpy_h2d(ctx_, p_, host, n * sizeof(T)));
        return st_->ok();
    }
    // the first n elements to host memory; nothing for a null host pointer
    bool download(T* host, size_t n) const
    {
        if (host && n && st_->ok()) (*st_)(les_hip_memcpy_d2h(ctx_, host, p_, n * sizeof(T)));
        return st_->ok();
    }

private:
    les_hip_ctx* ctx_;
    Status* st_;
    T* p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace les_host
