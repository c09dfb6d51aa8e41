// engine_stats.hip — fluid diagnostics of the 2D handle (include/fluidsim.h "fluid diagnostics"): fs_stats_read and
// fs_stats_device.  Off the step path and observing only: the arrays are read where fs_particles_device would export them from,
// and nothing of the handle's state changes but the scratch the first call allocates (fsd::StatsScratch, engine.h).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "engine.h"
#include "fs_stats.h"

using namespace fsd;

static_assert(FS_STATS_SHIFT == (int)STATS_SHIFT, "the header's shift is the kernels'");
static_assert(sizeof(fs_stats) == 208 && offsetof(fs_stats, count) == 0 && offsetof(fs_stats, nonfinite) == 8 &&
                  offsetof(fs_stats, dropped) == 16 && offsetof(fs_stats, momentum_q) == 24 && offsetof(fs_stats, energy_q) == 40 &&
                  offsetof(fs_stats, position_q) == 48 && offsetof(fs_stats, density_q) == 64 && offsetof(fs_stats, speed2_max) == 72 &&
                  offsetof(fs_stats, density_min) == 76 && offsetof(fs_stats, density_max) == 80 && offsetof(fs_stats, pos_min) == 84 &&
                  offsetof(fs_stats, pos_max) == 92 && offsetof(fs_stats, tick) == 100 && offsetof(fs_stats, attr_q) == 104 &&
                  offsetof(fs_stats, attr_dropped) == 136 && offsetof(fs_stats, attr_min) == 168 && offsetof(fs_stats, attr_max) == 184 &&
                  offsetof(fs_stats, channels) == 200 && offsetof(fs_stats, pad) == 204,
              "fs_stats is 208 bytes in the header's order");
// ... and the fold stores each word of a row where the header has its field (fs_stats.h)
static_assert(stats_word_offset(2, 0) == offsetof(fs_stats, momentum_q) && stats_word_offset(2, 2) == offsetof(fs_stats, energy_q) &&
                  stats_word_offset(2, 3) == offsetof(fs_stats, position_q) && stats_word_offset(2, 5) == offsetof(fs_stats, density_q) &&
                  stats_word_offset(2, 6) == offsetof(fs_stats, nonfinite) && stats_word_offset(2, 7) == offsetof(fs_stats, dropped) &&
                  stats_word_offset(2, 8) == offsetof(fs_stats, attr_q) && stats_word_offset(2, 12) == offsetof(fs_stats, attr_dropped) &&
                  stats_word_offset(2, 16) == offsetof(fs_stats, speed2_max) && stats_word_offset(2, 17) == offsetof(fs_stats, density_min) &&
                  stats_word_offset(2, 18) == offsetof(fs_stats, density_max) && stats_word_offset(2, 19) == offsetof(fs_stats, pos_min) &&
                  stats_word_offset(2, 21) == offsetof(fs_stats, pos_max) && stats_word_offset(2, 23) == offsetof(fs_stats, attr_min) &&
                  stats_word_offset(2, 27) == offsetof(fs_stats, attr_max) && stats_word_offset(2, 30) + 4 == offsetof(fs_stats, channels) &&
                  stats_attr_offset(2) - 4 == offsetof(fs_stats, tick),
              "a row's words land on the record's fields");

namespace {
// The three checks of both calls, in the header's order.
fs_status stats_check(const fs_sim* s, const void* out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "stats: single-domain handles only (not built for slab handles)");
    if (!out) return fail(FS_ERR_INVALID, "null argument");
    return FS_OK;
}

// Both launches on the simulation's stream, the record to `out_dev`.
fs_status stats_enqueue(fs_sim* s, fs_stats* out_dev) {
    FS_TRY(s->stats.reserve(2, sizeof(fs_stats)));
    StatsInput I;
    I.n = s->n; I.tick = s->tick;
    I.pos = s->pos.p; I.vel = s->vel.p;                      // fs_particles_device's export reads these ...
    I.rho = s->rho.p; I.rho2 = s->rho_in_rho2 ? s->rho2.p : nullptr;    // ... and finds the density here
    if (s->trk.channels > 0) {
        I.channels = s->trk.channels;
        I.attr = s->trk.channel(0, s->capacity); I.attr_stride = s->capacity;
    }
    launch_stats(s->stream, I, s->stats.slab.p, out_dev);
    FS_HIP(hipGetLastError());
    return FS_OK;
}
}  // namespace

extern "C" {

fs_status fs_stats_device(fs_sim* s, fs_stats* out_dev) {
    FS_TRY(stats_check(s, out_dev));
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    return stats_enqueue(s, out_dev);
}

fs_status fs_stats_read(fs_sim* s, fs_stats* out) {
    FS_TRY(stats_check(s, out));
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->stats.reserve(2, sizeof(fs_stats)));
    FS_TRY(s->stats.read(s->stream, out, [&](fs_stats* dev) { return stats_enqueue(s, dev); }));
    return sort_health(s);        // the record is in `out` either way; FS_ERR_DEVICE says the state it describes is not to be trusted
}

}  // extern "C"
