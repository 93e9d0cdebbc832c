// csrc/sepaihrd_host_util.h -- what the host side of the C ABI does the same way in every entry point: the error text, the
// choice of the device, the buffers of one call, the buffers a context keeps between calls, the copies of the results, the
// convergence diagnostics' checks.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "sepaihrd_device.h"
#include "sepaihrd_hip.h"

namespace sepaihrd {

inline void set_err(char* err, int errlen, const std::string& msg) {
    if (err && errlen > 0) std::snprintf(err, (size_t)errlen, "%s", msg.c_str());
}

// Pick and open the device of a context or of a one-off call: `device` < 0 stands for the current one and is replaced by its
// index.  SEPAIHRD_OK, or the code of the refusal with its text in err.
inline int select_device(int& device, char* err, int errlen) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_err(err, errlen, std::string("no HIP device available (this library has no CPU fallback): hipGetDeviceCount -> ") +
                                 hipGetErrorString(e) + ", count " + std::to_string(ndev));
        return SEPAIHRD_E_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) { set_err(err, errlen, "hipGetDevice failed"); return SEPAIHRD_E_HIP; }
    if (device >= ndev) { set_err(err, errlen, "device index out of range"); return SEPAIHRD_E_INVALID_ARG; }
    if (hipSetDevice(device) != hipSuccess) { set_err(err, errlen, "hipSetDevice failed"); return SEPAIHRD_E_HIP; }
    return SEPAIHRD_OK;
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

// an allocation that a HIP_TRY would have named: the same "<expression>: <what went wrong>" text for an owner's get / reserve
#define ALLOC_TRY(expr, ctx, fail)                                                           \
    do {                                                                                     \
        if (!(expr)) {                                                                       \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(hipErrorOutOfMemory); \
            fail;                                                                            \
        }                                                                                    \
    } while (0)

// ---- owners: every device buffer, page-locked buffer, event and stream is released by the destructor of exactly one of
// these.  The two memory kinds as (allocate, free) pairs, true for success; a failed allocation leaves HIP's error state clear.
inline bool device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess || ((void)hipGetLastError(), false); }
inline void device_free(void* p) { (void)hipFree(p); }
inline bool pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess || ((void)hipGetLastError(), false); }
inline void pinned_free(void* p) { (void)hipHostFree(p); }

// ONE grow-only buffer: get() hands it out, grown to `count` elements (at least 8 bytes) if it is smaller; false when the
// allocation fails (the buffer is then empty: nullptr, capacity 0).  Allocating tens of GB per call costs more than the
// kernels at large ensembles, hence grow-only.
template <bool (*Alloc)(void**, size_t), void (*Free)(void*)>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { release(); }
    bool reserve(size_t bytes) {
        bytes = std::max<size_t>(bytes, 8);
        if (cap >= bytes) return true;
        release();
        if (!Alloc(&p, bytes)) { p = nullptr; return false; }
        cap = bytes;
        return true;
    }
    template <class T>
    bool get(T** out, size_t count) {
        const bool ok = reserve(count * sizeof(T));
        *out = static_cast<T*>(p);
        return ok;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    void release() {
        if (p) Free(p);
        p = nullptr;
        cap = 0;
    }
};
using DeviceBuf = GrowBuf<device_alloc, device_free>;
using PinnedBuf = GrowBuf<pinned_alloc, pinned_free>;

// N buffers a context keeps between calls, one per role: get() is the slot's.
template <int N, class Buf = DeviceBuf>
struct GrowSlots {
    Buf slot[N];
    template <class T>
    bool get(int k, T** p, size_t count) { return slot[k].get(p, count); }
    void release() { for (Buf& b : slot) b.release(); }
};

// The allocations an object makes once and keeps for its lifetime.  alloc() yields a valid pointer even for count == 0, so
// that kernels may form it.
template <bool (*Alloc)(void**, size_t), void (*Free)(void*)>
struct FixedAllocs {
    std::vector<void*> bufs;
    FixedAllocs() = default;
    FixedAllocs(const FixedAllocs&) = delete;
    FixedAllocs& operator=(const FixedAllocs&) = delete;
    ~FixedAllocs() { for (void* b : bufs) Free(b); }
    bool bytes(void** p, size_t n) {
        if (!Alloc(p, n ? n : 1)) { *p = nullptr; return false; }
        bufs.push_back(*p);
        return true;
    }
    template <class T>
    bool alloc(T** p, size_t count) {
        void* q = nullptr;
        const bool ok = bytes(&q, (count ? count : 1) * sizeof(T));
        *p = static_cast<T*>(q);
        return ok;
    }
};
using DeviceAllocs = FixedAllocs<device_alloc, device_free>;
using PinnedAllocs = FixedAllocs<pinned_alloc, pinned_free>;

// a vector on the device for as long as `a` lives (one element when it is empty); a failure clears `ok`
template <class T>
const T* upload(DeviceAllocs& a, const std::vector<T>& v, bool& ok) {
    T* p = nullptr;
    if (!a.alloc(&p, v.size())) { ok = false; return nullptr; }
    if (!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return p;
}

// An event / a stream: a null handle until created, used wherever the raw handle is (the conversion).  &x is the address of
// the handle, so that a creation call inside a HIP_TRY reads -- and reports -- as it would with a raw handle.  A stream is
// drained before it is destroyed.
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
    Event& operator=(const Event&) = delete;
    ~Event() { if (h) (void)hipEventDestroy(h); }
    hipError_t create(unsigned flags) { const hipError_t e = hipEventCreateWithFlags(&h, flags); if (e != hipSuccess) h = nullptr; return e; }
    operator hipEvent_t() const { return h; }
    hipEvent_t* operator&() { return &h; }
};
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (h) { (void)hipStreamSynchronize(h); (void)hipStreamDestroy(h); } }
    hipError_t create(unsigned flags) { const hipError_t e = hipStreamCreateWithFlags(&h, flags); if (e != hipSuccess) h = nullptr; return e; }
    operator hipStream_t() const { return h; }
    hipStream_t* operator&() { return &h; }
};

// Device buffers, events and (where the call runs on a stream of its own) the stream of ONE call, released however the
// call ends.  The events are created by the caller (n_events null handles to fill), as is the stream.
// Release order (reverse of declaration): stream, events, buffers.
struct CallScratch {
    DeviceAllocs bufs;
    std::vector<Event> ev;
    Stream stream;
    explicit CallScratch(size_t n_events = 0) : ev(n_events) {}
    template <class T>
    bool alloc(T** p, size_t count) { return bufs.alloc(p, count); }
};

// the results of a call copied back: only those the caller asked for, nothing more after the first failure
struct ResultFetch {
    bool good = true;
    void fetch(void* dst, const void* src, size_t bytes) {
        if (good && dst && bytes && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) good = false;
    }
    bool ok() const { return good; }
};

// The device side of a probe (a one-off call that runs a few values through one kernel): in() allocates a buffer and uploads
// `count` values, out() allocates one.  When ready() the caller launches, then names what to copy back: the first fetch() asks
// for the launch's error and waits for the kernel.  status() is SEPAIHRD_OK, or SEPAIHRD_E_HIP with "<who>: <HIP's text>" in err
// (a failed allocation: hipErrorOutOfMemory's).
struct Probe {
    CallScratch sc;
    bool oom = false, good = true, launched = false;
    template <class T>
    T* out(size_t count) {
        T* p = nullptr;
        if (!oom && good && !sc.alloc(&p, count)) oom = true;
        return p;
    }
    template <class T>
    T* in(const T* host, size_t count) {
        T* p = out<T>(count);
        if (p && hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) good = false;
        return p;
    }
    bool ready() const { return !oom && good; }
    template <class T>
    void fetch(T* host, const T* dev, size_t count) {
        if (!launched) good = good && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        launched = true;
        good = good && hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
    }
    int status(const char* who, char* err, int errlen) const {
        if (ready()) return SEPAIHRD_OK;
        set_err(err, errlen, std::string(who) + ": " + hipGetErrorString(oom ? hipErrorOutOfMemory : hipGetLastError()));
        return SEPAIHRD_E_HIP;
    }
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

// The convergence diagnostics of a context's own samples (sepaihrd_chain_diagnostics) and of a sampler's (sepaihrd_mh_diagnostics):
// the shape both accept, and the run with its failures as the C ABI's codes.  Ctx: anything with last_error and pending_B.
// (static: an instantiation stays in the translation unit that asked for it)
template <class Ctx>
static int diag_check_shape(Ctx* ctx, const char* who, int C, int N, int P) {
    if (C < 1 || P < 1 || N < 4) {
        ctx->last_error = std::string(who) + ": need C >= 1 chains, P >= 1 columns and N >= 4 draws per chain";
        return SEPAIHRD_E_INVALID_ARG;
    }
    if ((int64_t)C * N >= ((int64_t)1 << 31)) {
        ctx->last_error = std::string(who) + ": C N must stay below 2^31 draws per column";
        return SEPAIHRD_E_INVALID_ARG;
    }
    if (ctx->pending_B > 0) {
        ctx->last_error = std::string(who) + ": a sepaihrd_eval_batch_begin is pending on this context";
        return SEPAIHRD_E_INVALID_ARG;
    }
    return SEPAIHRD_OK;
}
template <class Ctx>
static int diag_run(Ctx* ctx, const char* who, const DiagInput& in, double* out, int32_t* max_lag, hipStream_t st) {
    const int rc = chain_diagnostics(in, out, max_lag, st);
    if (rc == -4) { ctx->last_error = std::string(who) + ": invalid shape"; return SEPAIHRD_E_INVALID_ARG; }
    if (rc != 0) {
        const hipError_t e = hipGetLastError();
        ctx->last_error = std::string(who) + ": device failure (" + hipGetErrorString(e) + ")";
        return SEPAIHRD_E_HIP;
    }
    return SEPAIHRD_OK;
}

}  // namespace sepaihrd
