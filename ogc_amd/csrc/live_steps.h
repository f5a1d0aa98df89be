// live_steps.h — the live-step lists of a first level's neighbour lists: what the list forms of the chain's kernels share
// (backward: gn_fused_bwd.hip; forward: conv1x1.hip), and live_steps.hip, where live_steps_kernel makes the lists.
//
// A neighbour list idx (B, P, S) ends in repeats of its first entry wherever the search found fewer than S points inside the
// radius (utils/pointnet2_util.py:59-79).  Every kernel of a level's chain is column-wise, so those columns carry bit-equal
// values and gradients; only sums over positions see them, and there a weight stands for them.  Per centre
//     fill = 1 + max{ j : idx[j] != idx[0] }  (1: none),   T = S / 16,   s* = min(fill / 16, T - 1):
// steps 0 .. s* are LIVE, steps s* + 1 .. T - 1 are skipped; when s* < T - 1 the last column of step s* is a repeat (16 (s* + 1) >
// fill) and stands for itself and the 16 (T - 1 - s*) skipped columns.  The list of a sample: its live steps ascending, entry =
// position / 16, with the skipped-step count T - 1 - s* in the bits from LIVE_SHIFT up ON THE ENTRY OF STEP s* (zero on the
// others: the weight 1 + 16 * (entry >> LIVE_SHIFT) belongs to that step's last position alone); n[b] entries of `cap` are used.
//
// The FORWARD list holds the same entries in the same order, packed so that no GROUP — the entries of one 64-position tile of the
// dense kernels, entry >> 2: one centre at S = 64, a pair of centres at S = 32 — crosses a boundary between tiles of four entries:
// a group that does not fit the slots left in the current tile starts the next one, and the slots it leaves are LIVE_PAD
// (greedy).  Every tile holds at least one whole group, so hw / 16 entries still cover the worst case; n[b] counts the pads
// in front of the last entry, and whatever follows entry n[b] - 1 in its tile is read as a pad.  A wave of a forward list form
// owns one such tile: it holds all live entries of every dense tile it touches, and can rebuild that tile's fp32 partial sums.
#pragma once
#include <cstdint>
#include "ogc_common.h"

namespace {

constexpr int LIVE_SHIFT = 28;
constexpr int LIVE_MASK = (1 << LIVE_SHIFT) - 1;
constexpr int LIVE_PAD = -1; // forward list: an empty slot (every real entry is >= 0)
struct LiveIn {
    const int *steps = nullptr; // (B, cap)
    const int *n = nullptr;     // (B)
    int cap = 0;
};

// the list forms' own preconditions (checked ahead of every launch and memset): a list with room for the worst case, every step
// live — n_live stays on the device, so a list shorter than that could be shorter than n_live — and S = 32 or 64
inline int live_check(const char *name, const int *live, const int *n_live, int live_cap, int hw, int nsample, LiveIn &ls) {
    OGC_REQUIRE(live && n_live, "%s: null live-step list", name);
    if (nsample != 32 && nsample != 64) {
        ogc_set_error("%s: the list form needs nsample 32 or 64 (nsample=%d)", name, nsample);
        return OGC_ERR_UNSUPPORTED;
    }
    OGC_REQUIRE(hw >= 16 && hw % nsample == 0 && (hw >> 4) <= LIVE_MASK && live_cap >= (hw >> 4),
                "%s: the live-step list holds %d entries per sample, hw=%d needs room for %d", name, live_cap, hw, hw >> 4);
    ls.steps = live; ls.n = n_live; ls.cap = live_cap;
    return OGC_OK;
}

} // namespace
