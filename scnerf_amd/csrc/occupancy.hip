// occupancy.hip -- forward-only rendering skips the samples that lie in empty space (ops.inference_occupancy): the baking of
// an occupancy grid from the trained density, and the small kernels that put the unchanged network forward on the live
// samples of a pass.
//
// The grid: one bit per cell of an R x R x R lattice over the box [lo, hi), R a multiple of 32.  Cell (x, y, z) is bit
// c & 31 of word c >> 5, c = (z R + y) R + x; the words are int32.  A sample with point p is DEAD only when all three
// t_a = (p_a - lo_a) * inv_a -- one fp32 subtraction, one fp32 multiplication, each rounded, never fused -- satisfy
// 0 <= t_a < R and the bit of cell (floor t_x, floor t_y, floor t_z) is 0.  A NaN coordinate and a point outside the box are
// live.  inv_a = R / (hi_a - lo_a) is the caller's (computed once, in fp32, on the host).
//
//   occ_probe_kernel        cells [first, first + n) and k in {1, 2, 3} -> pts [n k^3][3], point q = (jz k + jy) k + jx of cell
//                           (x, y, z):  p_a = lo_a + ((float)i_a + off[j_a]) * cell_a,  an int -> fp32 conversion (exact), an fp32
//                           addition, an fp32 multiplication, an fp32 addition, each rounded, in this order;
//                           off[j] = (j + 0.5) / k and cell_a = (hi_a - lo_a) / R are the caller's fp32 numbers.
//   occ_accumulate_kernel   raw [n k^3][4], sigma_min -> the cells' bits OR-ed into the words.  One lane per cell; the cell is
//                           set when any of its probes has !(sigma <= sigma_min) -- a NaN density sets it.  The ballot of a
//                           wave is two words, lane 0 and lane 32 store one each: a word belongs to one wave (first is a
//                           multiple of 64), so the OR across networks and passes is that lane's read-modify-write.
//   occ_dilate_kernel       one round of 26-neighbourhood dilation, bits_in -> bits_out, one thread per word: the OR of the
//                           nine neighbouring rows (y, z; a grid edge has no neighbour), then in x the word, its two shifts
//                           and the carries from the two neighbouring words of the row.
//   occ_count_kernel / occ_scatter_kernel   pts [P][3] -> live_idx (ascending), slot_of [P] (-1 on a dead sample), the live
//                           points, one view direction per live sample (that of ray i / samples_per_ray) and the count, in
//                           device memory and in a pinned host word.  As csrc/live_compact.hip: a workgroup owns 1024
//                           consecutive samples, the first launch leaves one count per workgroup, the second sums the counts
//                           in front of it and every wave writes at base + (live lanes below).
//   occ_expand_raw_kernel   raw_live, slot_of -> raw [P][4], 16 bytes per sample, zero rows for the dead: every row written.
//
// Plain loads and stores and wave ballots; no atomic anywhere: every output is a function of the input alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.h"
#include "occ_cell.h"
#include "scn_wave.h"
#include "scnerf_hip.h"

namespace {

using namespace scn;

typedef unsigned words4 __attribute__((ext_vector_type(4)));       // 16 bytes moved as one

constexpr int kOccWaves = 4;
constexpr int kOccThreads = kOccWaves * kWave;
constexpr int kTilesPerWave = 4;
constexpr int kOccBlock = kOccThreads * kTilesPerWave;           // samples per workgroup

// the cell test of a sample and the once-rounded fp32 operations: occ_cell.h, shared with early_stop.hip
using occ::add_rn;
using occ::bad_resolution;
using occ::Grid;
using occ::mul_rn;
using occ::sample_live;

// sample i of wave w, tile k of workgroup b
__device__ __forceinline__ long sample_of(long b, int w, int k, int lane) {
    return b * kOccBlock + (w * kTilesPerWave + k) * kWave + lane;
}

__global__ __launch_bounds__(kOccThreads) void occ_count_kernel(Grid g, const float* __restrict__ pts, long P,
                                                                int* __restrict__ block_counts) {
    int* counts = dynamic_lds<int>();                       // [kOccWaves]
    const int lane = lane_id(), w = wave_id();
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        mine += popcount64(ballot(i < P && sample_live(g, pts, i)));
    }
    if (lane == 0) counts[w] = mine;
    block_sync();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = counts[0] + counts[1] + counts[2] + counts[3];
}

__global__ __launch_bounds__(kOccThreads) void occ_scatter_kernel(Grid g, const float* __restrict__ pts, long P,
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
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        live[k] = i < P && sample_live(g, pts, i);
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
            const long ray = i / samples_per_ray;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pts_live[3 * slot + c] = pts[3 * i + c];
                vd_live[3 * slot + c] = viewdirs[ray * vd_stride + c];
            }
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

__global__ __launch_bounds__(256) void occ_expand_raw_kernel(const float* __restrict__ raw_live, const int* __restrict__ slot_of,
                                                             float* __restrict__ raw, long P, long n_live) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const long slot = slot_of[i];
    words4 v = words4{0u, 0u, 0u, 0u};
    if (slot >= 0 && slot < n_live) v = *reinterpret_cast<const words4*>(raw_live + slot * 4);      // (no index followed unchecked)
    *reinterpret_cast<words4*>(raw + i * 4) = v;
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
__global__ __launch_bounds__(256) void occ_probe_kernel(ProbeArgs a, float* __restrict__ pts) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int k3 = a.k * a.k * a.k;
    if (e >= a.n_cells * k3) return;
    const long cl = e / k3;
    const int q = (int)(e - cl * k3);
    const int jx = q % a.k, jy = (q / a.k) % a.k, jz = q / (a.k * a.k);
    const long c = a.first + cl;
    const int x = (int)(c % a.R), y = (int)((c / a.R) % a.R), z = (int)(c / ((long)a.R * a.R));
    pts[3 * e + 0] = probe_coord(x, jx, a.lo_x, a.cell_x, a);
    pts[3 * e + 1] = probe_coord(y, jy, a.lo_y, a.cell_y, a);
    pts[3 * e + 2] = probe_coord(z, jz, a.lo_z, a.cell_z, a);
}

// one lane per cell, one wave per 64 cells = two words
__global__ __launch_bounds__(kOccThreads) void occ_accumulate_kernel(const float* __restrict__ raw, float sigma_min, long first,
                                                                     long n_cells, int k3, long n_words,
                                                                     unsigned* __restrict__ bits) {
    const int lane = lane_id();
    const long cl = ((long)blockIdx.x * kOccWaves + wave_id()) * kWave + lane;
    bool set = false;
    if (cl < n_cells) {
        for (int q = 0; q < k3; ++q) set = set || !(raw[(cl * k3 + q) * 4 + 3] <= sigma_min);       // (a NaN sets the cell)
    }
    const unsigned long long m = ballot(set);
    const long word = ((first + cl) >> 5);                  // lane 0: the wave's first word, lane 32: its second
    if ((lane & 31) == 0 && cl < n_cells && word < n_words) {
        const unsigned mine = lane == 0 ? (unsigned)m : (unsigned)(m >> 32);
        bits[word] = bits[word] | mine;
    }
}

// one thread per word
__global__ __launch_bounds__(256) void occ_dilate_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ out, int R) {
    const int wpr = R >> 5;                                 // words per row
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)R * R * wpr) return;
    const int wx = (int)(e % wpr);
    const long row = e / wpr;
    const int y = (int)(row % R), z = (int)(row / R);
    unsigned l = 0u, m = 0u, r = 0u;
    for (int dz = -1; dz <= 1; ++dz) {
        const int zz = z + dz;
        if (zz < 0 || zz >= R) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= R) continue;
            const unsigned* p = in + ((long)zz * R + yy) * wpr;
            m |= p[wx];
            if (wx > 0) l |= p[wx - 1];
            if (wx + 1 < wpr) r |= p[wx + 1];
        }
    }
    out[e] = m | (m << 1) | (m >> 1) | (l >> 31) | (r << 31);
}

}  // namespace

extern "C" long long scnerf_occ_compact_workspace_ints(long long n_samples) {
    return n_samples < 0 ? -1 : (long long)scn_ceil_div(n_samples > 0 ? n_samples : 1, kOccBlock);
}

extern "C" int scnerf_occ_compact(const float* pts, long long n_samples, const float* viewdirs, int vd_stride,
                                  int samples_per_ray, const int* bits, int R, float lo_x, float lo_y, float lo_z,
                                  float inv_x, float inv_y, float inv_z, int* workspace, int* live_idx, int* slot_of, float* pts_live, float* vd_live,
                                  int* n_live_dev, int* n_live_host, void* stream) {
    SCN_RETURN_IF(n_samples < 0 || n_samples > 0x7fffffffll || bad_resolution(R), SCN_EINVAL);
    SCN_RETURN_IF(!bits || !workspace || !n_live_dev || samples_per_ray < 1 || vd_stride < 3, SCN_EINVAL);
    SCN_RETURN_IF(n_samples > 0 && (!pts || !viewdirs || !live_idx || !slot_of || !pts_live || !vd_live), SCN_EINVAL);
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
    hipLaunchKernelGGL(occ_count_kernel, dim3(blocks), dim3(kOccThreads), kOccWaves * sizeof(int), st, g, pts, (long)n_samples,
                       workspace);
    const int rc = scn_launch_status();
    SCN_RETURN_IF(rc != 0, rc);
    hipLaunchKernelGGL(occ_scatter_kernel, dim3(blocks), dim3(kOccThreads), 2 * kOccWaves * sizeof(int), st, g, pts,
                       (long)n_samples, viewdirs, vd_stride, samples_per_ray, workspace, live_idx, slot_of, pts_live, vd_live,
                       n_live_dev, n_live_host);
    return scn_launch_status();
}

extern "C" int scnerf_occ_expand_raw(const float* raw_live, const int* slot_of, float* raw, long long n_samples,
                                     long long n_live, void* stream) {
    SCN_RETURN_IF(n_samples < 0 || n_samples > 0x7fffffffll || n_live < 0 || n_live > n_samples, SCN_EINVAL);
    if (n_samples == 0) return 0;
    SCN_RETURN_IF(!slot_of || !raw || (n_live > 0 && !raw_live), SCN_EINVAL);
    // rows move as 16-byte vectors
    SCN_RETURN_IF((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(raw_live)) & 15u, SCN_EINVAL);
    hipLaunchKernelGGL(occ_expand_raw_kernel, dim3(scn_ceil_div(n_samples, 256)), dim3(256), 0, (hipStream_t)stream, raw_live,
                       slot_of, raw, (long)n_samples, (long)n_live);
    return scn_launch_status();
}

static bool bad_cell_range(long long first, long long n_cells, int R) {
    const long long cells = (long long)R * R * R;
    return first < 0 || (first & 63) != 0 || n_cells < 0 || first + n_cells > cells;
}

extern "C" int scnerf_occ_probe_points(long long first_cell, long long n_cells, int R, int k, float lo_x, float lo_y,
                                       float lo_z, float cell_x, float cell_y, float cell_z, float off0, float off1,
                                       float off2, float* pts, void* stream) {
    SCN_RETURN_IF(bad_resolution(R) || k < 1 || k > 3 || bad_cell_range(first_cell, n_cells, R), SCN_EINVAL);
    SCN_RETURN_IF(n_cells * k * k * k > 0x7fffffffll, SCN_EINVAL);
    if (n_cells == 0) return 0;
    SCN_RETURN_IF(!pts, SCN_EINVAL);
    const ProbeArgs a{(long)first_cell, (long)n_cells, R, k, lo_x, lo_y, lo_z, cell_x, cell_y, cell_z, off0, off1, off2};
    hipLaunchKernelGGL(occ_probe_kernel, dim3(scn_ceil_div(n_cells * k * k * k, 256)), dim3(256), 0, (hipStream_t)stream, a, pts);
    return scn_launch_status();
}

extern "C" int scnerf_occ_accumulate(const float* raw, float sigma_min, long long first_cell, long long n_cells, int R, int k,
                                     int* bits, void* stream) {
    SCN_RETURN_IF(bad_resolution(R) || k < 1 || k > 3 || bad_cell_range(first_cell, n_cells, R), SCN_EINVAL);
    SCN_RETURN_IF(n_cells * k * k * k > 0x7fffffffll, SCN_EINVAL);
    if (n_cells == 0) return 0;
    SCN_RETURN_IF(!raw || !bits, SCN_EINVAL);
    const long n_words = (long)R * R * R / 32;
    hipLaunchKernelGGL(occ_accumulate_kernel, dim3(scn_ceil_div(n_cells, kOccThreads)), dim3(kOccThreads), 0, (hipStream_t)stream,
                       raw, sigma_min, (long)first_cell, (long)n_cells, k * k * k, n_words, reinterpret_cast<unsigned*>(bits));
    return scn_launch_status();
}

extern "C" int scnerf_occ_dilate(const int* bits_in, int* bits_out, int R, void* stream) {
    SCN_RETURN_IF(bad_resolution(R) || !bits_in || !bits_out || bits_in == bits_out, SCN_EINVAL);
    const long words = (long)R * R * (R >> 5);
    hipLaunchKernelGGL(occ_dilate_kernel, dim3(scn_ceil_div(words, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(bits_in), reinterpret_cast<unsigned*>(bits_out), R);
    return scn_launch_status();
}
