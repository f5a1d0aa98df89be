"""The rigid-ICP kernel source (ogc_amd/csrc/rigid_icp.hip + svd3.h) compiled for the HOST and run thread for thread — one OS
thread per GPU thread, std::barrier for __syncthreads, a barrier-guarded slot array for __shfl_down — on every case of
tests/golden/icp.npz.  Same IEEE double operations in the same order as on the device (no contraction, correctly rounded sqrt and
division), so it shows what the algorithm gives against the reference's values before any GPU is involved: iteration counts and
the largest deviations of T and of the distances per case.  It is a rehearsal, not a measurement of the device.

    python tools/icp_host_emulation.py        (needs g++ with C++20; ~15 s, up to 1024 threads)"""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ogc_amd", "csrc")

SHIM = r'''
// host emulation of the few HIP features rigid_icp.hip uses: one OS thread per GPU thread
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <thread>
#include <vector>
#include <barrier>
#include <algorithm>
#include <memory>
#include "ogc_ops.h"
#define OGC_WAVE 64
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float4 { float x, y, z, w; };
typedef void *hipStream_t;
extern thread_local dim3 threadIdx, blockIdx, blockDim;
extern char *smem;
struct Block { std::barrier<> *all; std::vector<std::unique_ptr<std::barrier<>>> waves; std::vector<double> slots; };
extern Block *g_block;
inline void __syncthreads() { g_block->all->arrive_and_wait(); }
inline double __shfl_down(double v, int off, int width) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    g_block->slots[threadIdx.x] = v;
    g_block->waves[wave]->arrive_and_wait();
    const double r = lane + off < width ? g_block->slots[wave * 64 + lane + off] : v;
    g_block->waves[wave]->arrive_and_wait();
    return r;
}
using std::min; using std::isfinite;
static char g_err[512];
#define OGC_REQUIRE(cond, ...) do { if (!(cond)) { snprintf(g_err, sizeof g_err, __VA_ARGS__); return OGC_ERR_INVALID_ARG; } } while (0)
#define OGC_CHECK_LAUNCH(name)
static inline int ogc_divup(long long a, long long b) { return (int)((a + b - 1) / b); }
template <class K, class... A>
void emu_launch(K kernel, dim3 grid, dim3 block, size_t lds, A... args) {
    for (unsigned b = 0; b < grid.x; ++b) {
        smem = (char *)aligned_alloc(16, (lds + 15) & ~(size_t)15);
        memset(smem, 0xAB, lds);
        Block blk; std::barrier<> all(block.x); blk.all = &all; blk.slots.resize(block.x);
        for (unsigned w = 0; w < block.x / 64; ++w) blk.waves.emplace_back(new std::barrier<>(64));
        g_block = &blk;
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t)
            ts.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); blockDim = block; kernel(args...); });
        for (auto &t : ts) t.join();
        free(smem);
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emu_launch(kernel, grid, block, lds, __VA_ARGS__)
'''


def build(workdir):
    def patched(name):
        text = open(os.path.join(CSRC, name)).read().replace('#include "ogc_common.h"', '#include "shim.h"')
        return text.replace("extern __shared__ __attribute__((aligned(16))) char smem[];", "")
    open(os.path.join(workdir, "shim.h"), "w").write(SHIM)
    open(os.path.join(workdir, "svd3.h"), "w").write(patched("svd3.h"))
    open(os.path.join(workdir, "rigid_icp_emu.cpp"), "w").write(
        '#include "shim.h"\nthread_local dim3 threadIdx, blockIdx, blockDim; char *smem; Block *g_block;\n' + patched("rigid_icp.hip"))
    lib = os.path.join(workdir, "libicp_emu.so")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + workdir,
                           "-pthread", "-shared", "-fPIC", os.path.join(workdir, "rigid_icp_emu.cpp"), "-o", lib])
    L = ctypes.CDLL(lib)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.ogc_rigid_icp.argtypes = [i, i, vp, vp, vp, i, d, vp, vp, vp, vp]
    return L


def run(L, src, dst, init, max_iterations, tolerance):
    B, n = src.shape[:2]
    T, dist, it = np.zeros((B, 4, 4)), np.zeros((B, n)), np.zeros(B, np.int32)
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    init = None if init is None else np.ascontiguousarray(init)
    rc = L.ogc_rigid_icp(B, n, src.ctypes.data, dst.ctypes.data, None if init is None else init.ctypes.data, max_iterations,
                         tolerance, T.ctypes.data, dist.ctypes.data, it.ctypes.data, None)
    assert rc == 0, rc
    return T, dist, it


def main():
    data = np.load(os.path.join(ROOT, "tests", "golden", "icp.npz"))
    meta = json.loads(str(data["meta"]))
    with tempfile.TemporaryDirectory() as workdir:
        L = build(workdir)
        worst = [0.0, 0.0, 0.0]
        for name, case in sorted(meta["cases"].items()):
            k = case["inputs"]
            src, dst = data[k + "_src"], data[k + "_dst"]
            init = data[k + "_init"] if case["has_init"] else None
            T, dist, it = run(L, src, dst, init, case["max_iterations"], case["tolerance"])
            again = run(L, src, dst, init, case["max_iterations"], case["tolerance"])
            both = np.concatenate([src, dst], 1)
            extent = float((both.max(1) - both.min(1)).max())
            rot = float(np.abs(T[:, :3, :3] - data[name + "_T"][:, :3, :3]).max())
            trans = float(np.abs(T[:, :3, 3] - data[name + "_T"][:, :3, 3]).max()) / extent
            dd = float(np.abs(dist - data[name + "_distances"]).max())
            worst = [max(a, b) for a, b in zip(worst, (rot, trans, dd))]
            print("%-3s iters %s (reference %s)  rot %.2e  trans/extent %.2e  distances %.2e  repeatable %s"
                  % (name, it.tolist(), data[name + "_iters"].tolist(), rot, trans, dd,
                     all(np.array_equal(a, b) for a, b in zip((T, dist, it), again))))
        print("largest: rot %.2e  trans/extent %.2e  distances %.2e" % tuple(worst))


if __name__ == "__main__":
    main()
