// fs_host.h — what the host files of the C ABI (engine*.hip) share: the last-error helper, the HIP error macro, and the
// owners of a handle's device arrays, streams, events and per-pass event ring.  Every owner frees what it holds in its
// destructor, so a handle is torn down by `delete` alone (members go in reverse order of declaration), and a blocking call
// stages device memory in DevArray locals: it synchronises the stream (or ends on a blocking copy) before they go out of scope.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fluidsim.h"

namespace fsd {

void set_last_error(const std::string& msg);   // what fs_last_error() returns on this thread (engine.hip)

inline fs_status fail(fs_status st, const std::string& msg) {
    set_last_error(msg);
    return st;
}

// Leave the calling function with a status and a message when a HIP call fails.
#define FS_HIP(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e__ = (expr);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            return fsd::fail(e__ == hipErrorOutOfMemory ? FS_ERR_OOM : FS_ERR_DEVICE,                    \
                             std::string(#expr) + ": " + hipGetErrorString(e__));                        \
        }                                                                                                \
    } while (0)

// ... and when a call that returns a status does not return FS_OK.
#define FS_TRY(expr) do { const fs_status r__ = (expr); if (r__ != FS_OK) return r__; } while (0)

// A device array: move-only, freed by the destructor (or at once by release()).
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t n = 0;
    DevArray() = default;
    DevArray(DevArray&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevArray& operator=(DevArray&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    ~DevArray() { release(); }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        return count ? hipMalloc((void**)&p, count * sizeof(T)) : hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// The blocking form of a point query (fs_sample_*, fs3_sample_*): device staging for the points (none: the query is a grid), the
// records (none: `out` is null, fs3_sample_attr_* without weights) and `ch` channel sums per point; `enqueue(points_dev, out_dev,
// attr_dev)` puts the kernel on `st` and returns a status.
template <class Pt, class Rec, class Enqueue>
fs_status staged_query(hipStream_t st, const Pt* points, size_t n, Rec* out, float* attr_out, size_t ch, Enqueue enqueue) {
    DevArray<Pt> dpts;
    DevArray<Rec> dout;
    DevArray<float> dattr;
    hipError_t e = points ? dpts.alloc(n) : hipSuccess;
    if (e == hipSuccess) e = dout.alloc(out ? n : 0);
    if (e == hipSuccess) e = dattr.alloc(ch * n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "sampling: device staging");
    }
    fs_status r = FS_OK;
    if (points) e = hipMemcpyAsync(dpts.p, points, n * sizeof(Pt), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        r = enqueue(dpts.p, dout.p, dattr.p);
        if (r == FS_OK && out) e = hipMemcpyAsync(out, dout.p, n * sizeof(Rec), hipMemcpyDeviceToHost, st);
        if (r == FS_OK && e == hipSuccess && ch) e = hipMemcpyAsync(attr_out, dattr.p, ch * n * sizeof(float), hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);      // before the staging is freed, whatever happened
    if (e == hipSuccess) e = es;
    if (r == FS_OK && e != hipSuccess) r = fail(FS_ERR_DEVICE, hipGetErrorString(e));
    return r;
}

// The blocking form of a call that only reads back what a kernel wrote (a G-buffer, counts, a mesh): device staging for `n`
// records, `enqueue(out_dev)` puts the kernel on `st` and returns a status, the records land in `out`.  As staged_query: no
// staging is FS_ERR_OOM, and the stream is synchronised before the staging is freed, whatever happened.
template <class Rec, class Enqueue>
fs_status download_records(hipStream_t st, size_t n, Rec* out, Enqueue enqueue) {
    DevArray<Rec> dout;
    if (dout.alloc(n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "sampling: device staging");
    }
    fs_status r = enqueue(dout.p);
    hipError_t e = r == FS_OK ? hipMemcpyAsync(out, dout.p, n * sizeof(Rec), hipMemcpyDeviceToHost, st) : hipSuccess;
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (r == FS_OK && e != hipSuccess) r = fail(FS_ERR_DEVICE, hipGetErrorString(e));
    return r;
}

// A stream or an event of a handle: created into `h` by the HIP call that fits, destroyed with its owner.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

static_assert(!std::is_copy_constructible<DevArray<float>>::value && !std::is_copy_assignable<DevArray<float>>::value &&
                  !std::is_copy_constructible<Stream>::value && !std::is_copy_constructible<Event>::value,
              "owners are never copied: two destructors would free one resource");

// Per-pass timing: a ring of event sets (FS_PASS_COUNT + 1 events per step) recorded on the stream; drained
// (synchronised and accumulated) only when read or when the ring is full, never per step.
struct PassRing {
    static const uint32_t RING = 256;
    bool on = false;                // fs_profile_enable / fs3_profile_enable
    std::vector<hipEvent_t> ev;     // RING * (FS_PASS_COUNT + 1), created by the first profiled step
    uint32_t pending = 0;           // steps recorded since the last drain
    double ms[FS_PASS_COUNT] = {};
    uint64_t steps = 0;

    PassRing() = default;
    PassRing(const PassRing&) = delete;
    PassRing& operator=(const PassRing&) = delete;
    ~PassRing() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }

    // the event set of the step being enqueued; `pending += 1` once its last event is recorded
    hipEvent_t* current() { return &ev[(size_t)pending * (FS_PASS_COUNT + 1)]; }
    // before the first event of a profiled step: a set is free (the ring exists, a full one has been drained)
    fs_status begin() {
        if (ev.empty()) {
            ev.resize((size_t)RING * (FS_PASS_COUNT + 1), nullptr);
            for (auto& e : ev) FS_HIP(hipEventCreate(&e));
        }
        return pending == RING ? drain() : FS_OK;
    }
    fs_status drain() {
        if (pending == 0) return FS_OK;
        const size_t stride = FS_PASS_COUNT + 1;
        FS_HIP(hipEventSynchronize(ev[(size_t)(pending - 1) * stride + FS_PASS_COUNT]));
        for (uint32_t j = 0; j < pending; ++j) {
            for (int k = 0; k < FS_PASS_COUNT; ++k) {
                float t = 0.0f;
                FS_HIP(hipEventElapsedTime(&t, ev[j * stride + k], ev[j * stride + k + 1]));
                ms[k] += t;
            }
        }
        steps += pending;
        pending = 0;
        return FS_OK;
    }
    // fs_profile_read / fs3_profile_read
    fs_status read(double out_ms[FS_PASS_COUNT], uint64_t* out_steps, int reset) {
        FS_TRY(drain());
        for (int k = 0; k < FS_PASS_COUNT; ++k) out_ms[k] = ms[k];
        if (out_steps) *out_steps = steps;
        if (reset) { for (auto& m : ms) m = 0.0; steps = 0; }
        return FS_OK;
    }
};

}  // namespace fsd
