// live_compact.hip -- the backward pass of a training step on the LIVE samples alone (ops.live_samples).
//
// raw2outputs forms alpha = 1 - exp(-relu(sigma + noise) * dist) (NeRF/run_nerf_helpers.py: raw2outputs).  A sample whose
// noisy density is not positive has alpha = 0 and weight 0 exactly, so its d_raw row is all +-0, and with it every dZ row of
// the sample, its input gradient and its term in every weight and bias gradient.  The small kernels here put the unchanged
// data-gradient kernel and the weight-gradient GEMMs on the other samples:
//
//   live_count_kernel / live_scatter_kernel   d_raw [P][4] -> live_idx (ascending original indices), the offset table the
//                           256 x 256 weight-gradient kernel gathers X through (wgrad256_half.h), the live d_raw rows and
//                           the count, in device memory and in a pinned host word.  A sample is live when any of its four
//                           words is non-zero with the sign bit ignored (a NaN is live).
//   live_gather_kernel      what mlp_bwd_h3_kernel reads for the compact batch: the nine lane-native mask sections, the
//                           points and one view direction per sample (the kernel then runs with samples_per_ray = 1).
//   live_remap_maxima_kernel  the forward's X chunk maxima -> the compact chunks: compact chunk c holds original samples
//                           live_idx[first] .. live_idx[last], its bound is the largest over the original chunks in that
//                           span -- an upper bound, all the scale needs.
//
// Order-preserving and without an atomic: a workgroup owns 1024 consecutive samples, the first launch leaves one count per
// workgroup, the second sums the counts in front of it (integers: any order) and every wave writes at base + (live lanes
// below).  Every output is a function of the input alone.  Entries of live_idx / the offset table between the count and
// its padding to 128 name sample 0 (offset 0): the consumers read them for rows whose dZ is zero.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch.h"
#include "mlp_common.h"
#include "scn_wave.h"
#include "scnerf_hip.h"

namespace {

using namespace scn;

typedef unsigned words4 __attribute__((ext_vector_type(4)));       // 16 bytes moved as one

constexpr int kLiveWaves = 4;
constexpr int kLiveThreads = kLiveWaves * kWave;
constexpr int kTilesPerWave = 4;
constexpr int kLiveBlock = kLiveThreads * kTilesPerWave;         // samples per workgroup
constexpr long long kLiveMaxSamples = (1LL << 22) - 128;         // 1 KB per sample and 256-wide section: offsets below 2^32

__device__ __forceinline__ bool row_live(const float* __restrict__ d_raw, long i) {
    const words4 w = *reinterpret_cast<const words4*>(d_raw + i * 4);
    return ((w.x | w.y | w.z | w.w) & 0x7fffffffu) != 0u;
}

// sample i of wave w, tile k of workgroup b
__device__ __forceinline__ long sample_of(int b, int w, int k, int lane) {
    return (long)b * kLiveBlock + (w * kTilesPerWave + k) * kWave + lane;
}

__global__ __launch_bounds__(kLiveThreads) void live_count_kernel(const float* __restrict__ d_raw, long P,
                                                                  int* __restrict__ block_counts) {
    int* counts = dynamic_lds<int>();                       // [kLiveWaves]
    const int lane = lane_id(), w = wave_id();
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        mine += popcount64(ballot(i < P && row_live(d_raw, i)));
    }
    if (lane == 0) counts[w] = mine;
    block_sync();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = counts[0] + counts[1] + counts[2] + counts[3];
}

// where compact sample k sits in the offset table: per 16-sample slab the samples (ml, ml + 8) of a lane adjacent
__device__ __forceinline__ long table_pos(long k) { return (k & ~15L) + 2 * (k & 7) + ((k >> 3) & 1); }

__global__ __launch_bounds__(kLiveThreads) void live_scatter_kernel(const float* __restrict__ d_raw, long P,
                                                                    const int* __restrict__ block_counts,
                                                                    int* __restrict__ live_idx, unsigned* __restrict__ xoff,
                                                                    float* __restrict__ d_raw_live, int* __restrict__ n_live_dev,
                                                                    int* n_live_host) {
    int* lds = dynamic_lds<int>();                          // [kLiveWaves] partial sums of the counts in front, [kLiveWaves] counts
    const int lane = lane_id(), w = wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    // the live samples in front of this workgroup
    int front = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kLiveThreads) front += block_counts[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) front += shfl_xor(front, o);
    bool live[kTilesPerWave];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        live[k] = i < P && row_live(d_raw, i);
        mine += popcount64(ballot(live[k]));
    }
    if (lane == 0) { lds[w] = front; lds[kLiveWaves + w] = mine; }
    block_sync();
    int base = 0, in_block = 0;
#pragma unroll
    for (int v = 0; v < kLiveWaves; ++v) {
        base += lds[v] + (v < w ? lds[kLiveWaves + v] : 0);
        in_block += lds[kLiveWaves + v];
    }
#pragma unroll
    for (int k = 0; k < kTilesPerWave; ++k) {
        const long i = sample_of(blockIdx.x, w, k, lane);
        const unsigned long long m = ballot(live[k]);
        const long slot = base + popcount64(m & below);
        if (live[k]) {
            live_idx[slot] = (int)i;
            xoff[table_pos(slot)] = (unsigned)(i >> 5) * 32768u + (unsigned)(i & 31) * 16u;
            *reinterpret_cast<words4*>(d_raw_live + slot * 4) = *reinterpret_cast<const words4*>(d_raw + i * 4);
        }
        base += popcount64(m);
    }
    if (blockIdx.x == gridDim.x - 1) {
        // the last workgroup knows the total: the two count words, and the entries up to the padded count
        int total = 0;
#pragma unroll
        for (int v = 0; v < kLiveWaves; ++v) total += lds[v];
        total += in_block;
        const long padded = mlp::padded_samples((long)total);
        for (long k = total + threadIdx.x; k < padded; k += kLiveThreads) {
            live_idx[k] = 0;
            xoff[table_pos(k)] = 0u;
        }
        if (threadIdx.x == 0) {
            *n_live_dev = total;
            if (n_live_host) *n_live_host = total;
        }
    }
}

struct GatherArgs {
    const int* live_idx;
    long n_live, P, Ppad, Ppad_live;
    const unsigned* masks;       // [9][Ppad / 32][64][4]
    const float* pts; int pd;
    const float* viewdirs; int vd_stride; int samples_per_ray;
    unsigned* masks_live;        // [9][Ppad_live / 32][64][4]
    float* pts_live;             // [n_live][pd]
    float* vd_live;              // [n_live][3]
};

// thread e = piece * Ppad_live + k: piece = 2 section + lane half, the 16 bytes of compact sample k in it (a sample behind
// the count, or an index outside the source, gets zeros); the threads of piece 0 also move the point and the direction
__global__ __launch_bounds__(256) void live_gather_kernel(GatherArgs a) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 18 * a.Ppad_live) return;
    const int piece = (int)(e / a.Ppad_live);
    const long k = e - piece * a.Ppad_live;
    const int sect = piece >> 1, h = piece & 1;
    long i = k < a.n_live ? (long)a.live_idx[k] : -1;
    if (i >= a.P) i = -1;
    words4 v = words4{0u, 0u, 0u, 0u};
    if (i >= 0) v = *reinterpret_cast<const words4*>(a.masks + (((long)sect * (a.Ppad / 32) + (i >> 5)) * 64 + 32 * h + (i & 31)) * 4);
    *reinterpret_cast<words4*>(a.masks_live + (((long)sect * (a.Ppad_live / 32) + (k >> 5)) * 64 + 32 * h + (k & 31)) * 4) = v;
    if (piece == 0 && i >= 0) {
        for (int c = 0; c < a.pd; ++c) a.pts_live[k * a.pd + c] = a.pts[i * a.pd + c];
        const long ray = i / a.samples_per_ray;
        for (int c = 0; c < 3; ++c) a.vd_live[k * 3 + c] = a.viewdirs[ray * a.vd_stride + c];
    }
}

// dst [n][w] (zeroed in front of this launch): row live_idx[k] = src row k -- the input gradient of the compact batch back
// in sample order, for the dense ray reduction
__global__ __launch_bounds__(256) void live_scatter_rows_kernel(const float* __restrict__ src, const int* __restrict__ live_idx,
                                                                float* __restrict__ dst, long n_live, int w, long n) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_live * w) return;
    const long k = e / w;
    const int c = (int)(e - k * w);
    const long i = live_idx[k];
    if (i >= 0 && i < n) dst[i * w + c] = src[e];
}

__global__ __launch_bounds__(64) void live_remap_maxima_kernel(const int* __restrict__ live_idx, long n_live,
                                                               const float* __restrict__ amax_src, int n_src, long chunk_src,
                                                               float* __restrict__ amax_dst, int n_dst, long chunk_dst, int rows) {
    const int c = blockIdx.x, row = threadIdx.x;
    if (row >= rows) return;
    const long first = (long)c * chunk_dst;
    float v = 0.f;
    // entries behind the count name sample 0: a chunk that reaches past the count also bounds that sample's X (its dZ rows
    // are zero there, but X scaled by a bound of 0 would overflow the fp16 planes)
    if (first + chunk_dst > n_live) v = amax_src[(long)row * n_src];
    if (first < n_live) {
        const long last = min(first + chunk_dst, n_live) - 1;
        const int o0 = (int)min((long)live_idx[first] / chunk_src, (long)n_src - 1);
        const int o1 = (int)min((long)live_idx[last] / chunk_src, (long)n_src - 1);
        for (int o = max(o0, 0); o <= o1; ++o) v = fmaxf(v, amax_src[(long)row * n_src + o]);
    }
    amax_dst[(long)row * n_dst + c] = v;
}

}  // namespace

extern "C" long long scnerf_live_compact_workspace_ints(long long n_samples) {
    return n_samples < 0 ? -1 : (long long)scn_ceil_div(n_samples > 0 ? n_samples : 1, kLiveBlock);
}

extern "C" int scnerf_live_compact(const float* d_raw, long long n_samples, int* workspace, int* live_idx, unsigned* xoff,
                                   float* d_raw_live, int* n_live_dev, int* n_live_host, void* stream) {
    SCN_RETURN_IF(n_samples < 1 || !d_raw || !workspace || !live_idx || !xoff || !d_raw_live || !n_live_dev, SCN_EINVAL);
    SCN_RETURN_IF(n_samples > kLiveMaxSamples, SCN_ENOSUP);
    SCN_RETURN_IF((reinterpret_cast<uintptr_t>(d_raw) | reinterpret_cast<uintptr_t>(d_raw_live)) & 15u, SCN_EINVAL);
    SCN_RETURN_IF(reinterpret_cast<uintptr_t>(xoff) & 7u, SCN_EINVAL);
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
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = scn_ceil_div(n_samples, kLiveBlock);
    hipLaunchKernelGGL(live_count_kernel, dim3(blocks), dim3(kLiveThreads), kLiveWaves * sizeof(int), st, d_raw, (long)n_samples,
                       workspace);
    const int rc = scn_launch_status();
    SCN_RETURN_IF(rc != 0, rc);
    hipLaunchKernelGGL(live_scatter_kernel, dim3(blocks), dim3(kLiveThreads), 2 * kLiveWaves * sizeof(int), st, d_raw,
                       (long)n_samples, workspace, live_idx, xoff, d_raw_live, n_live_dev, n_live_host);
    return scn_launch_status();
}

extern "C" int scnerf_live_gather(const int* live_idx, long long n_live, long long n_samples, const unsigned* masks,
                                  const float* pts, int pt_dims, const float* viewdirs, int vd_stride, int samples_per_ray,
                                  unsigned* masks_live, float* pts_live, float* vd_live, void* stream) {
    SCN_RETURN_IF(n_live < 0 || n_live > n_samples || n_samples > kLiveMaxSamples || (pt_dims != 3 && pt_dims != 4), SCN_EINVAL);
    SCN_RETURN_IF(samples_per_ray < 1 || vd_stride < 3, SCN_EINVAL);
    if (n_live == 0) return 0;
    SCN_RETURN_IF(!live_idx || !masks || !pts || !viewdirs || !masks_live || !pts_live || !vd_live, SCN_EINVAL);
    SCN_RETURN_IF((reinterpret_cast<uintptr_t>(masks) | reinterpret_cast<uintptr_t>(masks_live)) & 15u, SCN_EINVAL);
    const long Ppad_live = scn::mlp::padded_samples((long)n_live);
    const GatherArgs a{live_idx, (long)n_live, (long)n_samples, scn::mlp::padded_samples((long)n_samples), Ppad_live, masks,
                       pts, pt_dims, viewdirs, vd_stride, samples_per_ray, masks_live, pts_live, vd_live};
    hipLaunchKernelGGL(live_gather_kernel, dim3(scn_ceil_div(18 * Ppad_live, 256)), dim3(256), 0, (hipStream_t)stream, a);
    return scn_launch_status();
}

extern "C" int scnerf_live_scatter_rows(const float* src, const int* live_idx, float* dst, long long n_live, int w,
                                        long long n, void* stream) {
    SCN_RETURN_IF(n_live < 0 || n < 0 || n_live > n || n > kLiveMaxSamples || w < 1, SCN_EINVAL);
    if (n == 0) return 0;
    SCN_RETURN_IF(!dst || (n_live > 0 && (!src || !live_idx)), SCN_EINVAL);
    hipStream_t st = (hipStream_t)stream;
    SCN_HIP(hipMemsetAsync(dst, 0, (size_t)n * w * sizeof(float), st));
    if (n_live == 0) return 0;
    hipLaunchKernelGGL(live_scatter_rows_kernel, dim3(scn_ceil_div(n_live * w, 256)), dim3(256), 0, st, src, live_idx, dst,
                       (long)n_live, w, (long)n);
    return scn_launch_status();
}

extern "C" int scnerf_live_remap_maxima(const int* live_idx, long long n_live, const float* amax_src, int n_chunks_src,
                                        long long chunk_src, float* amax_dst, int n_chunks_dst, long long chunk_dst, int rows,
                                        void* stream) {
    SCN_RETURN_IF(!live_idx || !amax_src || !amax_dst || n_live < 1 || n_chunks_src < 1 || n_chunks_dst < 1, SCN_EINVAL);
    SCN_RETURN_IF(chunk_src < 1 || chunk_dst < 1 || rows < 1 || rows > 64, SCN_EINVAL);
    hipLaunchKernelGGL(live_remap_maxima_kernel, dim3(n_chunks_dst), dim3(64), 0, (hipStream_t)stream, live_idx, (long)n_live,
                       amax_src, n_chunks_src, (long)chunk_src, amax_dst, n_chunks_dst, (long)chunk_dst, rows);
    return scn_launch_status();
}
