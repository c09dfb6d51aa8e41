// engine_3d_stats.hip — fluid diagnostics of the 3D handle (include/fluidsim.h "3D fluid diagnostics"):
// fs3_stats_read and fs3_stats_device.  Off the step path and observing only: the arrays fs3_download_particles' export reads, in
// place; nothing of the handle's state changes but the scratch the first call allocates (fsd::StatsScratch, engine.h).
#include <hip/hip_runtime.h>

#include <cstddef>

#include "engine_3d.h"
#include "fs_stats.h"

using namespace fsd;

static_assert(sizeof(fs3_stats) == 232 && offsetof(fs3_stats, count) == 0 && offsetof(fs3_stats, nonfinite) == 8 &&
                  offsetof(fs3_stats, dropped) == 16 && offsetof(fs3_stats, momentum_q) == 24 && offsetof(fs3_stats, energy_q) == 48 &&
                  offsetof(fs3_stats, position_q) == 56 && offsetof(fs3_stats, density_q) == 80 && offsetof(fs3_stats, speed2_max) == 88 &&
                  offsetof(fs3_stats, density_min) == 92 && offsetof(fs3_stats, density_max) == 96 && offsetof(fs3_stats, pos_min) == 100 &&
                  offsetof(fs3_stats, pos_max) == 112 && offsetof(fs3_stats, tick) == 124 && offsetof(fs3_stats, attr_q) == 128 &&
                  offsetof(fs3_stats, attr_dropped) == 160 && offsetof(fs3_stats, attr_min) == 192 && offsetof(fs3_stats, attr_max) == 208 &&
                  offsetof(fs3_stats, channels) == 224 && offsetof(fs3_stats, pad) == 228,
              "fs3_stats is 232 bytes in the header's order");
// ... and the fold stores each word of a row where the header has its field (fs_stats.h)
static_assert(stats_word_offset(3, 0) == offsetof(fs3_stats, momentum_q) && stats_word_offset(3, 3) == offsetof(fs3_stats, energy_q) &&
                  stats_word_offset(3, 4) == offsetof(fs3_stats, position_q) && stats_word_offset(3, 7) == offsetof(fs3_stats, density_q) &&
                  stats_word_offset(3, 8) == offsetof(fs3_stats, nonfinite) && stats_word_offset(3, 9) == offsetof(fs3_stats, dropped) &&
                  stats_word_offset(3, 10) == offsetof(fs3_stats, attr_q) && stats_word_offset(3, 14) == offsetof(fs3_stats, attr_dropped) &&
                  stats_word_offset(3, 18) == offsetof(fs3_stats, speed2_max) && stats_word_offset(3, 19) == offsetof(fs3_stats, density_min) &&
                  stats_word_offset(3, 20) == offsetof(fs3_stats, density_max) && stats_word_offset(3, 21) == offsetof(fs3_stats, pos_min) &&
                  stats_word_offset(3, 24) == offsetof(fs3_stats, pos_max) && stats_word_offset(3, 27) == offsetof(fs3_stats, attr_min) &&
                  stats_word_offset(3, 31) == offsetof(fs3_stats, attr_max) && stats_word_offset(3, 34) + 4 == offsetof(fs3_stats, channels) &&
                  stats_attr_offset(3) - 4 == offsetof(fs3_stats, tick),
              "a row's words land on the record's fields");

namespace {
// Both launches on the simulation's stream, the record to `out_dev`.
fs_status stats3_enqueue(fs_sim3* s, fs3_stats* out_dev) {
    FS_TRY(s->stats.reserve(3, sizeof(fs3_stats)));
    const Arrays3 A = s->arrays();
    Stats3Input I;
    I.n = s->n; I.tick = s->tick;
    I.pos = A.pos; I.vel = A.vel; I.pred = A.pred;          // what launch3_export reads
    if (s->trk.channels > 0) {
        I.channels = s->trk.channels;
        I.attr = s->trk.channel(0, s->cap); I.attr_stride = s->cap;
    }
    launch3_stats(s->stream, I, s->stats.slab.p, out_dev);
    FS_HIP(hipGetLastError());
    return FS_OK;
}
}  // namespace

extern "C" {

fs_status fs3_stats_device(fs_sim3* s, fs3_stats* out_dev) {
    if (!s || !out_dev) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    return stats3_enqueue(s, out_dev);
}

fs_status fs3_stats_read(fs_sim3* s, fs3_stats* out) {
    if (!s || !out) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->stats.reserve(3, sizeof(fs3_stats)));
    FS_TRY(s->stats.read(s->stream, out, [&](fs3_stats* dev) { return stats3_enqueue(s, dev); }));
    return sort_health3(s);       // the record is in `out` either way
}

}  // extern "C"
