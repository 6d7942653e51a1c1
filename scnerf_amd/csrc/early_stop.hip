// early_stop.hip -- forward-only rendering stops a ray once it is opaque (ops.inference_early_stop): the small kernels
// that run the network of a call's final stage front to back in K depth segments.
//
// Segment k of a stage of S samples per ray holds the sample indices [b_k, b_k+1), b_k = (k S) / K; a launch is told
// first = b_k and len = b_k+1 - b_k.  Element e of a segment, e in [0, n len), is sample first + e % len of ray e / len:
// dense sample i = ray S + first + e % len, ascending in e.
//
//   seg_count_kernel / seg_scatter_kernel   the segment's samples whose ray is alive (alive[ray] != 0; no flags: every ray)
//                           and, with a grid, whose cell the grid does not call empty (occ_cell.h) -> live_idx (the dense
//                           indices i, ascending), slot_of [n len] (-1 on a sample that does not run), the live points, one
//                           view direction per live sample and two counts -- the live samples, the alive rays -- in device
//                           memory and in pinned host words.  As occupancy.hip's compaction: a workgroup owns 1024
//                           consecutive elements, the first launch leaves its counts, the second sums the counts in front.
//   seg_expand_raw_kernel   raw_live, slot_of -> the segment's rows of the dense raw [n][S][4], 16 bytes per sample, zero
//                           rows for the samples that did not run: every row of the segment written, none outside it.
//   seg_transmittance_kernel   one wave per ray, four rays per workgroup (composite.hip's shape): the ray's transmittance
//                           behind segment k, T = T * prod q_i over the segment, q of ray::sample_terms (noise 0, `last`
//                           for sample S - 1 alone), multiplied in fp64 by ray::wave_incl_prod.  A ray is STOPPED when
//                           T <= eps, coded as alive = !(T <= eps): a NaN T stays alive.  Segment 0 reads neither T nor
//                           alive and writes T, alive and stop_segment (K, or 1 for a stopped ray) of every ray; a later
//                           segment touches the alive rays alone and sets stop_segment = k + 1 where one stops.
//
// Plain loads and stores, wave ballots and shuffles; no atomic anywhere: every output is a function of the input alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.h"
#include "occ_cell.h"
#include "ray_stage.h"
#include "scn_wave.h"
#include "scnerf_hip.h"

namespace {

using namespace scn;
using occ::Grid;

typedef unsigned words4 __attribute__((ext_vector_type(4)));       // 16 bytes moved as one

constexpr int kSegWaves = 4;
constexpr int kSegThreads = kSegWaves * kWave;
constexpr int kTilesPerWave = 4;
constexpr int kSegBlock = kSegThreads * kTilesPerWave;           // elements per workgroup
constexpr int kRaysPerBlock = 4;

struct Segment {
    long n_elems;                // n * len
    int S, first, len;
    const int* alive;            // [n] or null: every ray
    bool has_grid;
};

// element e of wave w, tile k of workgroup b
__device__ __forceinline__ long elem_of(long b, int w, int k, int lane) {
    return b * kSegBlock + (w * kTilesPerWave + k) * kWave + lane;
}

// -> the element runs; *i its dense sample index, *ray its ray, *heads: it is the first of an alive ray's segment
__device__ __forceinline__ bool elem_live(const Segment& s, const Grid& g, const float* __restrict__ pts, long e, long* i,
                                          long* ray, bool* heads) {
    *heads = false;
    if (e >= s.n_elems) return false;
    const long r = e / s.len;
    const int j = (int)(e - r * s.len);
    *ray = r;
    *i = r * s.S + s.first + j;
    const bool up = s.alive ? s.alive[r] != 0 : true;
    *heads = up && j == 0;
    if (!up) return false;
    return s.has_grid ? occ::sample_live(g, pts, *i) : true;
}

__global__ __launch_bounds__(kSegThreads) void seg_count_kernel(Segment s, Grid g, const float* __restrict__ pts, int n_blocks,
                                                                int* __restrict__ block_counts) {
    int* counts = dynamic_lds<int>();                       // [kSegWaves] samples, [kSegWaves] rays
    const int lane = lane_id(), w = wave_id();
    int mine = 0, rays = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        long i, ray;
        bool heads;
        const bool live = elem_live(s, g, pts, elem_of(blockIdx.x, w, k, lane), &i, &ray, &heads);
        mine += popcount64(ballot(live));
        rays += popcount64(ballot(heads));
    }
    if (lane == 0) { counts[w] = mine; counts[kSegWaves + w] = rays; }
    block_sync();
    if (threadIdx.x == 0) {
        block_counts[blockIdx.x] = counts[0] + counts[1] + counts[2] + counts[3];
        block_counts[n_blocks + blockIdx.x] = counts[4] + counts[5] + counts[6] + counts[7];
    }
}

__global__ __launch_bounds__(kSegThreads) void seg_scatter_kernel(Segment s, Grid g, const float* __restrict__ pts,
                                                                  const float* __restrict__ viewdirs, int vd_stride, int n_blocks,
                                                                  const int* __restrict__ block_counts,
                                                                  int* __restrict__ live_idx, int* __restrict__ slot_of,
                                                                  float* __restrict__ pts_live, float* __restrict__ vd_live,
                                                                  int* __restrict__ counts_dev, int* counts_host) {
    int* lds = dynamic_lds<int>();                          // [kSegWaves] partial sums of the counts in front, [kSegWaves] counts
    const int lane = lane_id(), w = wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool last_block = (int)blockIdx.x == n_blocks - 1;
    // the live samples in front of this workgroup; the last workgroup also sums the alive rays of all the others
    int front = 0, rays_front = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kSegThreads) {
        front += block_counts[b];
        if (last_block) rays_front += block_counts[n_blocks + b];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        front += shfl_xor(front, o);
        rays_front += shfl_xor(rays_front, o);
    }
    bool live[kTilesPerWave];
    long idx[kTilesPerWave], ray_of[kTilesPerWave];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        bool heads;
        idx[k] = 0;
        ray_of[k] = 0;
        live[k] = elem_live(s, g, pts, elem_of(blockIdx.x, w, k, lane), &idx[k], &ray_of[k], &heads);
        mine += popcount64(ballot(live[k]));
    }
    if (lane == 0) { lds[w] = front; lds[kSegWaves + w] = mine; lds[2 * kSegWaves + w] = rays_front; }
    block_sync();
    int base = 0, in_block = 0;
#pragma unroll
    for (int v = 0; v < kSegWaves; ++v) {
        base += lds[v] + (v < w ? lds[kSegWaves + v] : 0);
        in_block += lds[kSegWaves + v];
    }
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long e = elem_of(blockIdx.x, w, k, lane);
        const unsigned long long m = ballot(live[k]);
        const long slot = base + popcount64(m & below);
        if (live[k]) {
            const long i = idx[k];
            live_idx[slot] = (int)i;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pts_live[3 * slot + c] = pts[3 * i + c];
                vd_live[3 * slot + c] = viewdirs[ray_of[k] * vd_stride + c];
            }
        }
        if (e < s.n_elems) slot_of[e] = live[k] ? (int)slot : -1;
        base += popcount64(m);
    }
    if (last_block && threadIdx.x == 0) {
        // the last workgroup knows the totals: the two pairs of count words
        int total = in_block, rays = block_counts[2 * n_blocks - 1];
#pragma unroll
        for (int v = 0; v < kSegWaves; ++v) { total += lds[v]; rays += lds[2 * kSegWaves + v]; }
        counts_dev[0] = total;
        counts_dev[1] = rays;
        if (counts_host) { counts_host[0] = total; counts_host[1] = rays; }
    }
}

__global__ __launch_bounds__(256) void seg_expand_raw_kernel(const float* __restrict__ raw_live, const int* __restrict__ slot_of,
                                                             float* __restrict__ raw, long n_elems, int S, int first, int len,
                                                             long n_live) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems) return;
    const long ray = e / len;
    const long i = ray * S + first + (e - ray * len);
    const long slot = slot_of[e];
    words4 v = words4{0u, 0u, 0u, 0u};
    if (slot >= 0 && slot < n_live) v = *reinterpret_cast<const words4*>(raw_live + slot * 4);      // (no index followed unchecked)
    *reinterpret_cast<words4*>(raw + i * 4) = v;
}

__global__ __launch_bounds__(256) void seg_transmittance_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                const float* __restrict__ rays, int ray_stride, int n, int S,
                                                                int first, int end, int k, int K, double eps,
                                                                double* __restrict__ T, int* __restrict__ alive,
                                                                int* __restrict__ stop_segment) {
    const int lane = lane_id();
    const int ray = blockIdx.x * kRaysPerBlock + wave_id();
    const bool opening = k == 0;
    // (the whole wave leaves: no barrier follows) a stopped ray keeps what it has
    if (ray >= n || !(opening || alive[ray] != 0)) return;
    const float norm = ray::ray_norm(rays + (size_t)ray * ray_stride + 3);
    const float* rr = raw + (size_t)ray * S * 4;
    const float* zr = z + (size_t)ray * S;
    double carry = opening ? 1.0 : T[ray];
    for (int base = first; base < end; base += 64) {
        const int i = base + lane;
        const bool in = i < end;
        const int ic = in ? i : end - 1;
        const float zi = zr[ic];
        const float zn = ic + 1 < S ? zr[ic + 1] : zi;
        const ray::SampleTerms t = ray::sample_terms(rr[(size_t)ic * 4 + 3], 0.f, zi, zn, ic == S - 1, norm);
        const double incl = ray::wave_incl_prod(in ? (double)t.q : 1.0, lane) * carry;
        carry = shfl(incl, 63);
    }
    if (lane == 0) {
        const bool up = !(carry <= eps);                    // (a NaN transmittance does not stop a ray)
        T[ray] = carry;
        alive[ray] = up ? 1 : 0;
        if (opening) stop_segment[ray] = up ? K : 1;
        else if (!up) stop_segment[ray] = k + 1;
    }
}

bool bad_segment(long long n, int S, int first, int len) {
    return n < 0 || S < 1 || first < 0 || len < 1 || first > S - len || n * (long long)S > 0x7fffffffll;
}

}  // namespace

extern "C" long long scnerf_seg_compact_workspace_ints(long long n_elems) {
    return n_elems < 0 ? -1 : 2 * (long long)scn_ceil_div(n_elems > 0 ? n_elems : 1, kSegBlock);
}

extern "C" int scnerf_seg_compact(const float* pts, long long n, int samples_per_ray, int first, int len, const int* alive,
                                  const float* viewdirs, int vd_stride, const int* bits, int R, float lo_x, float lo_y,
                                  float lo_z, float inv_x, float inv_y, float inv_z, int* workspace, int* live_idx,
                                  int* slot_of, float* pts_live, float* vd_live, int* counts_dev, int* counts_host,
                                  void* stream) {
    SCN_RETURN_IF(bad_segment(n, samples_per_ray, first, len) || vd_stride < 3 || !workspace || !counts_dev, SCN_EINVAL);
    SCN_RETURN_IF(bits && occ::bad_resolution(R), SCN_EINVAL);
    SCN_RETURN_IF(n > 0 && (!pts || !viewdirs || !live_idx || !slot_of || !pts_live || !vd_live), SCN_EINVAL);
#if !defined(SCNERF_SIMT_EMU_BUILD)
    if (counts_host) {
        // the kernel stores through this pointer: it must be page-locked memory the device can reach
        void* mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, counts_host, 0) != hipSuccess || !mapped) {
            (void)hipGetLastError();
            return SCN_EINVAL;
        }
        counts_host = static_cast<int*>(mapped);
    }
#endif
    const long n_elems = (long)n * len;
    const Segment s{n_elems, samples_per_ray, first, len, alive, bits != nullptr};
    const Grid g{reinterpret_cast<const unsigned*>(bits), R, lo_x, lo_y, lo_z, inv_x, inv_y, inv_z};
    hipStream_t st = (hipStream_t)stream;
    // (no element launches too: the count words are outputs)
    const unsigned blocks = scn_ceil_div(n_elems > 0 ? n_elems : 1, kSegBlock);
    hipLaunchKernelGGL(seg_count_kernel, dim3(blocks), dim3(kSegThreads), 2 * kSegWaves * sizeof(int), st, s, g, pts, (int)blocks,
                       workspace);
    const int rc = scn_launch_status();
    SCN_RETURN_IF(rc != 0, rc);
    hipLaunchKernelGGL(seg_scatter_kernel, dim3(blocks), dim3(kSegThreads), 3 * kSegWaves * sizeof(int), st, s, g, pts, viewdirs,
                       vd_stride, (int)blocks, workspace, live_idx, slot_of, pts_live, vd_live, counts_dev, counts_host);
    return scn_launch_status();
}

extern "C" int scnerf_seg_expand_raw(const float* raw_live, const int* slot_of, float* raw, long long n, int samples_per_ray,
                                     int first, int len, long long n_live, void* stream) {
    SCN_RETURN_IF(bad_segment(n, samples_per_ray, first, len) || n_live < 0 || n_live > n * len, SCN_EINVAL);
    if (n == 0) return 0;
    SCN_RETURN_IF(!slot_of || !raw || (n_live > 0 && !raw_live), SCN_EINVAL);
    // rows move as 16-byte vectors
    SCN_RETURN_IF((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(raw_live)) & 15u, SCN_EINVAL);
    const long n_elems = (long)n * len;
    hipLaunchKernelGGL(seg_expand_raw_kernel, dim3(scn_ceil_div(n_elems, 256)), dim3(256), 0, (hipStream_t)stream, raw_live,
                       slot_of, raw, n_elems, samples_per_ray, first, len, (long)n_live);
    return scn_launch_status();
}

extern "C" int scnerf_seg_transmittance(const float* raw, const float* z, const float* rays, int ray_stride, long long n,
                                        int samples_per_ray, int first, int len, int k, int K, double eps, double* T,
                                        int* alive, int* stop_segment, void* stream) {
    SCN_RETURN_IF(bad_segment(n, samples_per_ray, first, len) || ray_stride < 6 || k < 0 || K < 1 || k >= K, SCN_EINVAL);
    SCN_RETURN_IF(!(eps > 0.0 && eps < 1.0), SCN_EINVAL);
    if (n == 0) return 0;
    SCN_RETURN_IF(!raw || !z || !rays || !T || !alive || !stop_segment, SCN_EINVAL);
    hipLaunchKernelGGL(seg_transmittance_kernel, dim3(scn_ceil_div(n, kRaysPerBlock)), dim3(256), 0, (hipStream_t)stream, raw, z,
                       rays, ray_stride, (int)n, samples_per_ray, first, first + len, k, K, eps, T, alive, stop_segment);
    return scn_launch_status();
}
