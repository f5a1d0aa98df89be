// launch_shape.h — host-side pieces shared by the gather / group / interpolate families (gather_group.hip, group_linear.hip,
// group_reverse.hip, interpolate.hip): the opening of an entry point over (npoints, nsample) neighbour lists and the ladders
// that size a launch.
#pragma once
#include "ogc_common.h"

constexpr int GG_THREADS = 256; // workgroup of the gather, scatter-add and grouped-first-layer kernels

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The opening of an entry point over neighbour lists: `dims_ok` (the entry point's own dimension conditions) and the list shape
// are checked ("<name>: bad dimensions") and *T = npoints * nsample.  The caller decides what is empty.
static inline int group_open(const char *name, bool dims_ok, int npoints, int nsample, int *T) {
    *T = 0;
    OGC_REQUIRE(dims_ok && npoints >= 0 && nsample >= 0 && (long long)npoints * nsample < (1ll << 31), "%s: bad dimensions", name);
    *T = npoints * nsample;
    return OGC_OK;
}

// channels per workgroup of a kernel whose thread walks a slab of channels with one set of indices
static inline int pick_ch_per_block(int b, int c, int blocks_x) {
    // aim for >= ~2048 workgroups (8 per CU) before giving each workgroup more channels
    int cpb = 1;
    while (cpb < c && (long long)b * blocks_x * ((c + 2 * cpb - 1) / (2 * cpb)) >= 2048) cpb *= 2;
    return cpb;
}

// channel images per workgroup of an LDS-privatised scatter-add: as many images of n floats as `budget` floats hold, rounded
// down to 8 / 4 / 2 / 1, and no more than the c channels can fill
static inline int lds_image_channels(int budget, int n, int c) {
    int cc = budget / n;
    if (cc < 1) cc = 1;
    cc = cc >= 8 ? 8 : (cc >= 4 ? 4 : (cc >= 2 ? 2 : 1));
    while (cc > 1 && cc / 2 >= c) cc /= 2;
    return cc;
}
