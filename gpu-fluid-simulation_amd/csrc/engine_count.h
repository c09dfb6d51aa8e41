// engine_count.h — what engine_count.hip (the 2D handle) and engine_3d_count.hip (the 3D handle) share of a particle count that
// changes at run time, beyond Tracking::emitted and RemoveScratch in engine.h: plain functions over the
// pieces of a handle they work on.  Each handle's file keeps its entry points, its array lists and what it invalidates.
#pragma once
#include <utility>

#include "engine.h"

namespace fsd {

const uint32_t MAX_SLOTS = 1u << 28;       // as fs_create_ex / fs3_create: 32-bit byte offsets

inline uint32_t padded(uint32_t n) { uint32_t p2 = 1; while (p2 < n) p2 <<= 1; return p2; }

// device -> device on the handle's stream, `count` elements
template <class T>
hipError_t carry(hipStream_t st, DevArray<T>& to, const DevArray<T>& from, size_t count) {
    return count && from.p ? hipMemcpyAsync(to.p, from.p, count * sizeof(T), hipMemcpyDeviceToDevice, st) : hipSuccess;
}

// Tracking's share of a reserve, in the three phases of the caller's all-or-nothing scheme: everything new first (both id sets
// when ids exist, both channel sets for the channels allocated), the set in use copied behind the steps in flight (channel c
// moves from c * old_cap to c * cap), and — after the one synchronise, nothing having failed — the new arrays into the handle.
struct TrackingGrowth {
    DevArray<uint32_t> id[2];
    DevArray<float> attr[2];
    hipError_t alloc(const Tracking& T, size_t cap) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2 && e == hipSuccess; ++k) e = id[k].alloc(T.id[0].p ? cap : 0);
        for (int k = 0; k < 2 && e == hipSuccess; ++k) e = attr[k].alloc((size_t)T.alloc_channels * cap);
        return e;
    }
    hipError_t carry_from(hipStream_t q, const Tracking& T, size_t n, size_t old_cap, size_t cap) {
        if (!T.on()) return hipSuccess;
        hipError_t e = carry(q, id[T.cur], T.id[T.cur], n);
        for (int c = 0; c < T.channels && e == hipSuccess && n; ++c)
            e = hipMemcpyAsync(attr[T.cur].p + (size_t)c * cap, T.attr[T.cur].p + (size_t)c * old_cap, n * sizeof(float), hipMemcpyDeviceToDevice, q);
        return e;
    }
    void commit(Tracking& T) {
        if (id[0].p) { T.id[0] = std::move(id[0]); T.id[1] = std::move(id[1]); }
        if (attr[0].p) { T.attr[0] = std::move(attr[0]); T.attr[1] = std::move(attr[1]); }
    }
};

// The bitonic sort's bookkeeping of a count change old_n -> new_n; `dirty`: the handle's tile flags and plan
// words.  Inside one padded size the plan words stay where they are and the change is an upload to the policy.  Across one — and
// on every shrink, which blocks anyway — the plan words move: the stream is drained, the time-out word is read at its old place
// (the latch survives), all of `dirty` goes back to its state at create, and the policy starts over.  Returns the sort's health.
inline fs_status sort_count_changed(hipStream_t st, SortPolicy& sortp, DevArray<uint32_t>& dirty, uint32_t old_n, uint32_t new_n) {
    if (padded(new_n) == padded(old_n) && new_n >= old_n) {
        sortp.touched();
        return FS_OK;
    }
    FS_HIP(hipStreamSynchronize(st));
    const fs_status health = sortp.health(dirty.p, old_n);  // with the old count; latches SortPolicy::dead
    FS_HIP(hipMemsetAsync(dirty.p, 0, dirty.n * 4, st));
    sortp.resized();
    return health;
}

// A removal whose flags and offsets passes are enqueued on `st`: *keep = the survivors among n.  Blocking.  sortp: the policy
// of a handle that sorts with the bitonic network (its health is reported as wherever state is handed over), else null.
// FS_OK with *keep == n: nothing matched, and nothing is to change.
inline fs_status removal_survivors(hipStream_t st, const RemoveScratch& R, uint32_t n, SortPolicy* sortp, const uint32_t* dirty,
                                   uint32_t* keep) {
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(keep, R.sums.p + remove_workgroups(n), 4, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    if (sortp) FS_TRY(sortp->health(dirty, n));
    if (*keep != n && *keep < 2u) return fail(FS_ERR_INVALID, "removal: fewer than 2 particles would survive");
    return FS_OK;
}

// Tracking's fields of a scatter's argument (Compact2, Compact3): the set in use into the other one.  Off: they stay null.
template <class Compact>
void compact_tracking(Compact* C, const Tracking& T, uint32_t capacity) {
    if (!T.on()) return;
    C->ids = T.id[T.cur].p; C->ids_out = T.id[T.cur ^ 1].p;
    C->attr = T.attr[T.cur].p; C->attr_out = T.attr[T.cur ^ 1].p;
    C->channels = T.channels; C->stride = capacity;
}

}  // namespace fsd
