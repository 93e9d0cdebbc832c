// csrc/sepaihrd_host_util.h -- what the host side of the C ABI does the same way in every entry point: the error text, the
// buffers of one call, the buffers a context keeps between calls, the copies of the results.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "sepaihrd_hip.h"

namespace sepaihrd {

inline void set_err(char* err, int errlen, const std::string& msg) {
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", msg.c_str());
}

inline bool probabilities_valid(const double* probs, int n_probs) {
    for (int p = 0; p < n_probs; ++p)
        if (!(probs[p] >= 0.0 && probs[p] <= 1.0)) return false;
    return true;
}

// ctx: anything with a std::string last_error
#define HIP_TRY(expr, ctx, fail)                                                             \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);           \
            fail;                                                                            \
        }                                                                                    \
    } while (0)

// Device buffers, events and (where the call runs on a stream of its own) the stream of ONE call, released however the
// call ends.  The events are created by the caller (n_events null handles to fill), as is the stream.
struct CallScratch {
    std::vector<void*> bufs;
    std::vector<hipEvent_t> ev;
    hipStream_t stream = nullptr;
    explicit CallScratch(size_t n_events = 0) : ev(n_events, nullptr) {}
    CallScratch(const CallScratch&) = delete;
    CallScratch& operator=(const CallScratch&) = delete;
    ~CallScratch() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (void* b : bufs) if (b) (void)hipFree(b);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    // a valid pointer even for count == 0, so that kernels may form it
    template <class T>
    bool alloc(T** p, size_t count) {
        void* q = nullptr;
        if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
        bufs.push_back(q);
        *p = static_cast<T*>(q);
        return true;
    }
};

// N device buffers a context keeps between calls, one per role, grow-only: allocating tens of GB per call costs more than
// the kernels at large ensembles.  get() hands out the slot's buffer, grown to `count` elements (at least 8 bytes) if it is
// smaller; false when the allocation fails (the slot is then empty and the error state cleared).
template <int N>
struct GrowSlots {
    void* buf[N] = {};
    size_t cap[N] = {};
    template <class T>
    bool get(int slot, T** p, size_t count) {
        const size_t bytes = std::max<size_t>(count * sizeof(T), 8);
        if (cap[slot] < bytes) {
            if (buf[slot]) (void)hipFree(buf[slot]);
            buf[slot] = nullptr;
            cap[slot] = 0;
            if (hipMalloc(&buf[slot], bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
            cap[slot] = bytes;
        }
        *p = static_cast<T*>(buf[slot]);
        return true;
    }
    void release() {
        for (int k = 0; k < N; ++k) {
            if (buf[k]) (void)hipFree(buf[k]);
            buf[k] = nullptr;
            cap[k] = 0;
        }
    }
};

// the results of a call copied back: only those the caller asked for, nothing more after the first failure
struct ResultFetch {
    bool good = true;
    void fetch(void* dst, const void* src, size_t bytes) {
        if (good && dst && bytes && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) good = false;
    }
    bool ok() const { return good; }
};

// The buffers of a call must fit the device's memory; a larger request is refused before anything is allocated, with
// "<what> <need> MiB of device memory, the device has <total> MiB: <advice>" as the context's last error.
template <class Ctx>
int require_device_memory(Ctx* ctx, size_t need_bytes, const std::string& what, const char* advice) {
    size_t device_bytes = 0;
    HIP_TRY(hipDeviceTotalMem(&device_bytes, ctx->device), ctx, return SEPAIHRD_E_HIP);
    if (need_bytes <= device_bytes) return SEPAIHRD_OK;
    ctx->last_error = what + " " + std::to_string(need_bytes >> 20) + " MiB of device memory, the device has " +
                      std::to_string(device_bytes >> 20) + " MiB: " + advice;
    return SEPAIHRD_E_INVALID_ARG;
}

}  // namespace sepaihrd
