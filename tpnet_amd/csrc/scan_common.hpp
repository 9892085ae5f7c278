// Scan + compaction over one flag per element, shared by the tables that are built from head flags (negsampler.hip: the negative
// sampler's unique edges and candidates; edgebank.hip: EdgeBank's unique edges and its count of distinct edges per prefix).
// Tiles of 256 elements, one per thread, and a second level over the tile sums.  n = *n_dev when given (a count that lives on the
// device), else n_host.  k_scan_count: blk[tile] = flags set in the tile; k_scan_blocks (ONE workgroup, chunks of 256 tile sums with
// a running carry): blk -> exclusive, *total = the sum; k_scan_emit: position of a set flag = blk[tile] + its exclusive rank inside
// the tile.
#pragma once
#include "draw_common.hpp"

namespace tpnet {

template <class Flag>
__global__ __launch_bounds__(256) void k_scan_count(Flag f, const uint32_t* n_dev, uint32_t n_host, uint32_t* __restrict__ blk) {
    __shared__ uint32_t sh[4];
    const uint32_t n = n_dev ? *n_dev : n_host;
    const uint32_t nb = (n + 255u) / 256u;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint32_t j = tile * 256u + threadIdx.x;
        const uint32_t v = j < n ? f(j) : 0u;
        uint32_t tot;
        wg_scan256(v, sh, tot);
        if (threadIdx.x == 0) blk[tile] = tot;
    }
}

// (static: not a template, so every translation unit that includes this header gets a copy of its own)
static __global__ __launch_bounds__(256) void k_scan_blocks(uint32_t* __restrict__ blk, const uint32_t* n_dev, uint32_t n_host,
                                                            uint32_t* __restrict__ total) {
    __shared__ uint32_t sh[4];
    const uint32_t n = n_dev ? *n_dev : n_host;
    const uint32_t nb = (n + 255u) / 256u;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += 256u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? blk[i] : 0u;
        uint32_t tot;
        const uint32_t incl = wg_scan256(v, sh, tot);
        if (i < nb) blk[i] = carry + incl - v;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <class Flag, class Emit>
__global__ __launch_bounds__(256) void k_scan_emit(Flag f, Emit e, const uint32_t* n_dev, uint32_t n_host,
                                                   const uint32_t* __restrict__ blk) {
    __shared__ uint32_t sh[4];
    const uint32_t n = n_dev ? *n_dev : n_host;
    const uint32_t nb = (n + 255u) / 256u;
    for (uint32_t tile = blockIdx.x; tile < nb; tile += gridDim.x) {
        const uint32_t j = tile * 256u + threadIdx.x;
        const uint32_t v = j < n ? f(j) : 0u;
        uint32_t tot;
        const uint32_t incl = wg_scan256(v, sh, tot);
        if (v) e(j, blk[tile] + incl - v);
    }
}

// Host side, on stream s.  scan_count: the two launches that leave the exclusive tile sums in blk and the number of set flags in
// *total; scan_compact: those and k_scan_emit on the same flag.
template <class Flag>
static void scan_count(Flag f, const uint32_t* n_dev, uint32_t n_host, uint32_t* blk, uint32_t* total, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_scan_count<Flag>, dim3(grid), dim3(256), 0, s, f, n_dev, n_host, blk);
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(256), 0, s, blk, n_dev, n_host, total);
}
template <class Flag, class Emit>
static void scan_compact(Flag f, Emit e, const uint32_t* n_dev, uint32_t n_host, uint32_t* blk, uint32_t* total, int grid,
                         hipStream_t s) {
    scan_count(f, n_dev, n_host, blk, total, grid, s);
    hipLaunchKernelGGL((k_scan_emit<Flag, Emit>), dim3(grid), dim3(256), 0, s, f, e, n_dev, n_host, (const uint32_t*)blk);
}

}  // namespace tpnet
