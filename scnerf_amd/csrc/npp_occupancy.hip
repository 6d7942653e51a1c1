// npp_occupancy.hip -- forward-only NerfNet.forward calls (NeRF++) skip both networks on the samples that lie in empty space
// (ops.inference_occupancy_nerfpp).  The foreground network's grid is occupancy.hip's (euclidean, pts [P][3]); this file
// holds what the background network's grid needs on 4-D samples (x', y', z', w): a unit direction and w = 1 / r in [0, 1].
//
// The inverted-sphere space: q = (x' w, y' w, z' w) maps the outside of the unit sphere onto the unit ball; the grid is
// occupancy.hip's bit lattice over a box [lo, hi) in q.  A sample is DEAD only when q -- one fp32 multiplication per axis,
// rounded once -- lies inside the box and the bit of its cell is 0 (occ_cell.h, sample_live_inverted): a NaN component and
// a q outside the box are live.
//
//   occ_probe_inverted_kernel   cells [first, first + n) and k in {1, 2, 3} -> pts [n k^3][4]: the lattice point q of
//                               occ_probe_kernel (the same formula), then r2 = ((qx qx) + (qy qy)) + (qz qz), r = sqrt(r2),
//                               the probe (qx / r, qy / r, qz / r, min(r, 1)), every operation fp32 and correctly rounded;
//                               r == 0 gives (0, 0, 1, 0).  A lattice point outside the ball is probed on the sphere.
//   occ4_count_kernel / occ4_scatter_kernel   pts [P][4] -> live_idx (ascending), slot_of [P] (-1 on a dead sample), the live
//                               rows, one view direction per live sample (that of ray i / samples_per_ray) and the count, in
//                               device memory and in a pinned host word.  The scheme of occ_count_kernel / occ_scatter_kernel:
//                               a workgroup owns 1024 consecutive samples, the first launch leaves one count per workgroup,
//                               the second sums the counts in front of it and every wave writes at base + (live lanes
//                               below).  A point row moves as one 16-byte load and one 16-byte store.
//
// Plain loads and stores and wave ballots; no atomic anywhere: every output is a function of the input alone.  The raw rows
// are [P][4] in both spaces: scnerf_occ_expand_raw expands them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "launch.h"
#include "occ_cell.h"
#include "scn_wave.h"
#include "scnerf_hip.h"

namespace {

using namespace scn;

typedef unsigned row4 __attribute__((ext_vector_type(4)));        // a point row: 16 bytes moved as one

constexpr int kOccWaves = 4;
constexpr int kOccThreads = kOccWaves * kWave;
constexpr int kTilesPerWave = 4;
constexpr int kOccBlock = kOccThreads * kTilesPerWave;            // samples per workgroup

using occ::add_rn;
using occ::bad_resolution;
using occ::Grid;
using occ::mul_rn;
using occ::sample_live_inverted;

__device__ __forceinline__ float as_float(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned as_bits(float f) { return __builtin_bit_cast(unsigned, f); }

// sample i of wave w, tile k of workgroup b
__device__ __forceinline__ long sample_of(long b, int w, int k, int lane) {
    return b * kOccBlock + (w * kTilesPerWave + k) * kWave + lane;
}

__device__ __forceinline__ row4 row_of(const float* __restrict__ pts, long i) {
    return *reinterpret_cast<const row4*>(pts + 4 * i);
}

__device__ __forceinline__ bool row_live(const Grid& g, row4 p) {
    return sample_live_inverted(g, as_float(p.x), as_float(p.y), as_float(p.z), as_float(p.w));
}

__global__ __launch_bounds__(kOccThreads) void occ4_count_kernel(Grid g, const float* __restrict__ pts, long P,
                                                                 int* __restrict__ block_counts) {
    int* counts = dynamic_lds<int>();                       // [kOccWaves]
    const int lane = lane_id(), w = wave_id();
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        mine += popcount64(ballot(i < P && row_live(g, row_of(pts, i))));
    }
    if (lane == 0) counts[w] = mine;
    block_sync();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = counts[0] + counts[1] + counts[2] + counts[3];
}

__global__ __launch_bounds__(kOccThreads) void occ4_scatter_kernel(Grid g, const float* __restrict__ pts, long P,
                                                                   const float* __restrict__ viewdirs, int vd_stride,
                                                                   int samples_per_ray, const int* __restrict__ block_counts,
                                                                   int* __restrict__ live_idx, int* __restrict__ slot_of,
                                                                   float* __restrict__ pts_live, float* __restrict__ vd_live,
                                                                   int* __restrict__ n_live_dev, int* n_live_host) {
    int* lds = dynamic_lds<int>();                          // [kOccWaves] partial sums of the counts in front, [kOccWaves] counts
    const int lane = lane_id(), w = wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    // the live samples in front of this workgroup
    int front = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kOccThreads) front += block_counts[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) front += shfl_xor(front, o);
    bool live[kTilesPerWave];
    row4 row[kTilesPerWave];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        row[k] = row4{0u, 0u, 0u, 0u};
        if (i < P) row[k] = row_of(pts, i);
        live[k] = i < P && row_live(g, row[k]);
        mine += popcount64(ballot(live[k]));
    }
    if (lane == 0) { lds[w] = front; lds[kOccWaves + w] = mine; }
    block_sync();
    int base = 0, in_block = 0;
#pragma unroll
    for (int v = 0; v < kOccWaves; ++v) {
        base += lds[v] + (v < w ? lds[kOccWaves + v] : 0);
        in_block += lds[kOccWaves + v];
    }
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        const unsigned long long m = ballot(live[k]);
        const long slot = base + popcount64(m & below);
        if (live[k]) {
            live_idx[slot] = (int)i;
            *reinterpret_cast<row4*>(pts_live + 4 * slot) = row[k];
            const long ray = i / samples_per_ray;
#pragma unroll
            for (int c = 0; c < 3; ++c) vd_live[3 * slot + c] = viewdirs[ray * vd_stride + c];
        }
        if (i < P) slot_of[i] = live[k] ? (int)slot : -1;
        base += popcount64(m);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        // the last workgroup knows the total: the two count words
        int total = in_block;
#pragma unroll
        for (int v = 0; v < kOccWaves; ++v) total += lds[v];
        *n_live_dev = total;
        if (n_live_host) *n_live_host = total;
    }
}

struct ProbeArgs {
    long first, n_cells;
    int R, k;
    float lo_x, lo_y, lo_z, cell_x, cell_y, cell_z, off0, off1, off2;
};

__device__ __forceinline__ float probe_coord(int i, int j, float lo, float cell, const ProbeArgs& a) {
    const float off = j == 0 ? a.off0 : (j == 1 ? a.off1 : a.off2);
    return add_rn(lo, mul_rn(add_rn((float)i, off), cell));
}

// one thread per probe point
__global__ __launch_bounds__(256) void occ_probe_inverted_kernel(ProbeArgs a, float* __restrict__ pts) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int k3 = a.k * a.k * a.k;
    if (e >= a.n_cells * k3) return;
    const long cl = e / k3;
    const int q = (int)(e - cl * k3);
    const int jx = q % a.k, jy = (q / a.k) % a.k, jz = q / (a.k * a.k);
    const long c = a.first + cl;
    const int x = (int)(c % a.R), y = (int)((c / a.R) % a.R), z = (int)(c / ((long)a.R * a.R));
    const float qx = probe_coord(x, jx, a.lo_x, a.cell_x, a);
    const float qy = probe_coord(y, jy, a.lo_y, a.cell_y, a);
    const float qz = probe_coord(z, jz, a.lo_z, a.cell_z, a);
    const float r2 = add_rn(add_rn(mul_rn(qx, qx), mul_rn(qy, qy)), mul_rn(qz, qz));
    const float r = sqrtf(r2);                               // (correctly rounded: the build runs without fast math)
    row4 p = row4{0u, 0u, as_bits(1.f), 0u};
    if (!(r == 0.f)) p = row4{as_bits(qx / r), as_bits(qy / r), as_bits(qz / r), as_bits(r < 1.f ? r : 1.f)};
    *reinterpret_cast<row4*>(pts + 4 * e) = p;
}

static bool bad_cell_range(long long first, long long n_cells, int R) {
    const long long cells = (long long)R * R * R;
    return first < 0 || (first & 63) != 0 || n_cells < 0 || first + n_cells > cells;
}

}  // namespace

extern "C" long long scnerf_occ_compact4_workspace_ints(long long n_samples) {
    return n_samples < 0 ? -1 : (long long)scn_ceil_div(n_samples > 0 ? n_samples : 1, kOccBlock);
}

extern "C" int scnerf_occ_compact4(const float* pts, long long n_samples, const float* viewdirs, int vd_stride,
                                   int samples_per_ray, const int* bits, int R, float lo_x, float lo_y, float lo_z,
                                   float inv_x, float inv_y, float inv_z, int* workspace, int* live_idx, int* slot_of,
                                   float* pts_live, float* vd_live, int* n_live_dev, int* n_live_host, void* stream) {
    SCN_RETURN_IF(n_samples < 0 || n_samples > 0x7fffffffll || bad_resolution(R), SCN_EINVAL);
    SCN_RETURN_IF(!bits || !workspace || !n_live_dev || samples_per_ray < 1 || vd_stride < 3, SCN_EINVAL);
    SCN_RETURN_IF(n_samples > 0 && (!pts || !viewdirs || !live_idx || !slot_of || !pts_live || !vd_live), SCN_EINVAL);
    // rows move as 16-byte vectors
    SCN_RETURN_IF((reinterpret_cast<uintptr_t>(pts) | reinterpret_cast<uintptr_t>(pts_live)) & 15u, SCN_EINVAL);
#if !defined(SCNERF_SIMT_EMU_BUILD)
    if (n_live_host) {
        // the kernel stores through this pointer: it must be page-locked memory the device can reach
        void* mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, n_live_host, 0) != hipSuccess || !mapped) {
            (void)hipGetLastError();
            return SCN_EINVAL;
        }
        n_live_host = static_cast<int*>(mapped);
    }
#endif
    const Grid g{reinterpret_cast<const unsigned*>(bits), R, lo_x, lo_y, lo_z, inv_x, inv_y, inv_z};
    hipStream_t st = (hipStream_t)stream;
    // (no sample launches too: the two count words are outputs)
    const unsigned blocks = scn_ceil_div(n_samples > 0 ? n_samples : 1, kOccBlock);
    hipLaunchKernelGGL(occ4_count_kernel, dim3(blocks), dim3(kOccThreads), kOccWaves * sizeof(int), st, g, pts, (long)n_samples,
                       workspace);
    const int rc = scn_launch_status();
    SCN_RETURN_IF(rc != 0, rc);
    hipLaunchKernelGGL(occ4_scatter_kernel, dim3(blocks), dim3(kOccThreads), 2 * kOccWaves * sizeof(int), st, g, pts,
                       (long)n_samples, viewdirs, vd_stride, samples_per_ray, workspace, live_idx, slot_of, pts_live, vd_live,
                       n_live_dev, n_live_host);
    return scn_launch_status();
}

extern "C" int scnerf_occ_probe_points_inverted(long long first_cell, long long n_cells, int R, int k, float lo_x, float lo_y,
                                                float lo_z, float cell_x, float cell_y, float cell_z, float off0, float off1,
                                                float off2, float* pts, void* stream) {
    SCN_RETURN_IF(bad_resolution(R) || k < 1 || k > 3 || bad_cell_range(first_cell, n_cells, R), SCN_EINVAL);
    SCN_RETURN_IF(n_cells * k * k * k > 0x7fffffffll, SCN_EINVAL);
    if (n_cells == 0) return 0;
    SCN_RETURN_IF(!pts || (reinterpret_cast<uintptr_t>(pts) & 15u), SCN_EINVAL);
    const ProbeArgs a{(long)first_cell, (long)n_cells, R, k, lo_x, lo_y, lo_z, cell_x, cell_y, cell_z, off0, off1, off2};
    hipLaunchKernelGGL(occ_probe_inverted_kernel, dim3(scn_ceil_div(n_cells * k * k * k, 256)), dim3(256), 0, (hipStream_t)stream,
                       a, pts);
    return scn_launch_status();
}
