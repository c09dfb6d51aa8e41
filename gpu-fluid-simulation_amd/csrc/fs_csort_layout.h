// fs_csort_layout.h — where the counting sort (kernels_csort.hip) keeps what in its scratch.  Host arithmetic only, no HIP: the
// launchers include it, and so does the stand-alone check tests/emit2d_host_check.cpp (built with the host sanitizers).
//
//   hist (ncell + 1) | kt (slots x u64) | slot_src (slots) | scan state (u64 per scan tile) | ticket
//
// `slots` is what the scratch was sized for — a slab handle's or a strip's capacity, a single-domain handle's capacity — never a
// live count: the look-back words are epoch-stamped and never cleared and the ticket must be zero between steps, so neither may
// move when the count does.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fsd {

static const uint32_t CS_SCAN_TILE = 1024u * 16u;      // items per workgroup of k_scan_lookback (SCAN_BLOCK x SCAN_ITEMS)

static inline size_t cs_even(size_t w) { return (w + 1u) & ~(size_t)1u; }

struct CsLayout {
    uint32_t *hist, *slot_src, *ticket;
    unsigned long long *kt, *state;
    uint32_t scan_blocks;
};

static inline CsLayout cs_layout(uint32_t* scratch, uint32_t slots, uint32_t ncell) {
    CsLayout L;
    size_t o = 0;
    L.hist = scratch; o = cs_even((size_t)ncell + 1u);
    L.kt = (unsigned long long*)(scratch + o); o += 2 * (size_t)slots;
    L.slot_src = scratch + o; o = cs_even(o + slots);
    L.scan_blocks = (uint32_t)(((size_t)ncell + 1u + CS_SCAN_TILE - 1) / CS_SCAN_TILE);
    L.state = (unsigned long long*)(scratch + o); o += 2 * (size_t)L.scan_blocks;
    L.ticket = scratch + o;
    return L;
}

// Words to allocate; `ncell_max`: the largest table the handle will ever scan (slab handles move their window).
static inline size_t cs_scratch_words(uint32_t slots, uint32_t ncell_max) {
    const size_t tiles = ((size_t)ncell_max + 1u + CS_SCAN_TILE - 1) / CS_SCAN_TILE;
    return cs_even((size_t)ncell_max + 1u) + 2 * (size_t)slots + cs_even(slots) + 2 * tiles + 16;
}

}  // namespace fsd
