// ray_compact.hip -- forward-only rendering skips the fine pass of rays the coarse pass found empty
// (ops.inference_skip_empty): the three small kernels around the unchanged fine stage.
//
//   ray_compact_kernel      acc[n], tau -> live_idx (ascending), slot_of[n], n_live.  Ray i is skipped iff acc[i] <= tau
//                           (a NaN is therefore live).
//   ray_rows_gather_kernel  dst[j, :] = src[live_idx[j], :] -- the live rows of rays, z_c, w_c, u, noise.
//   ray_expand_kernel       the fine stage's outputs on the live batch -> full-size outputs; a skipped ray takes the coarse
//                           stage's per-ray values, z_std = 0 and zero rows.  Every element of every output is written:
//                           no memset in front.
//
// The compaction is ONE workgroup of 16 waves: wave w owns the w-th contiguous sixteenth of the rays (whole 64-ray tiles),
// counts its live rays (a ballot per tile), the sixteen counts meet in LDS behind one barrier, and the wave walks its
// segment a second time writing at base(w) + (live lanes below this one).  No atomic anywhere: every output is a function
// of the input alone.  A chunk of rays is a few 10^4 (render.py's `chunk`), 32 tiles per wave and pass; 2^24 rays are
// 16 384 tiles per wave, still without a barrier inside the loops.  The tile loops load four tiles before the first ballot
// so that the loads are in flight together.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scn_wave.h"
#include "scnerf_hip.h"

namespace {

using namespace scn;

constexpr int kCompactWaves = 16;
constexpr int kCompactThreads = kCompactWaves * kWave;
constexpr int kTilesInFlight = 4;

__global__ __launch_bounds__(kCompactThreads) void ray_compact_kernel(const float* __restrict__ acc, float tau,
                                                                      int* __restrict__ live_idx, int* __restrict__ slot_of,
                                                                      int* __restrict__ n_live_dev, int* n_live_host, long n) {
    int* counts = dynamic_lds<int>();                       // [kCompactWaves]
    const int lane = lane_id(), w = wave_id();
    const long tiles = (n + kWave - 1) / kWave;
    const long seg = (tiles + kCompactWaves - 1) / kCompactWaves * kWave;
    const long begin = seg * w < n ? seg * w : n, end = seg * (w + 1) < n ? seg * (w + 1) : n;
    const unsigned long long below = (1ull << lane) - 1ull;

    int mine = 0;
    for (long i0 = begin; i0 < end; i0 += kTilesInFlight * kWave) {
        bool live[kTilesInFlight];
#pragma unroll
        for (int k = 0; k < kTilesInFlight; ++k) {
            const long i = i0 + k * kWave + lane;
            live[k] = i < end && !(acc[i] <= tau);
        }
#pragma unroll
        for (int k = 0; k < kTilesInFlight; ++k) mine += popcount64(ballot(live[k]));
    }
    if (lane == 0) counts[w] = mine;
    block_sync();
    int base = 0, total = 0;
    for (int v = 0; v < kCompactWaves; ++v) {
        const int c = counts[v];
        base += v < w ? c : 0;
        total += c;
    }

    for (long i0 = begin; i0 < end; i0 += kTilesInFlight * kWave) {
        bool live[kTilesInFlight];
#pragma unroll
        for (int k = 0; k < kTilesInFlight; ++k) {
            const long i = i0 + k * kWave + lane;
            live[k] = i < end && !(acc[i] <= tau);
        }
#pragma unroll
        for (int k = 0; k < kTilesInFlight; ++k) {
            const long i = i0 + k * kWave + lane;
            const unsigned long long m = ballot(live[k]);
            const int slot = base + popcount64(m & below);
            if (live[k]) live_idx[slot] = (int)i;
            if (i < end) slot_of[i] = live[k] ? slot : -1;
            base += popcount64(m);
        }
    }
    if (threadIdx.x == 0) {
        *n_live_dev = total;
        if (n_live_host) *n_live_host = total;
    }
}

__global__ __launch_bounds__(256) void ray_rows_gather_kernel(const float* __restrict__ src, const int* __restrict__ live_idx,
                                                              float* __restrict__ dst, long n_live, int w, long n_src) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_live * w) return;
    const long j = e / w;
    const int c = (int)(e - j * w);
    const long i = live_idx[j];
    dst[e] = (i >= 0 && i < n_src) ? src[i * w + c] : 0.f;          // (an index outside the source is never followed)
}

struct ExpandArgs {
    const int* slot_of;
    // the fine stage on the live batch: [n_live, ...]
    const float *rgb_l, *disp_l, *acc_l, *depth_l, *z_std_l, *raw_l, *z_vals_l, *z_samples_l;
    // the coarse stage on every ray: [n, ...]
    const float *rgb0, *disp0, *acc0, *depth0;
    // full size
    float *rgb_map, *disp_map, *acc_map, *depth_map, *z_std, *raw, *z_vals, *z_samples;
    long n, n_live;
    int s_tot, s_fine;
};

constexpr int kExpandWaves = 4;

// one wave per ray
__global__ __launch_bounds__(kExpandWaves * kWave) void ray_expand_kernel(ExpandArgs a) {
    const long r = (long)blockIdx.x * kExpandWaves + wave_id();
    if (r >= a.n) return;
    const int lane = lane_id();
    const long slot = a.slot_of[r];
    const bool live = slot >= 0 && slot < a.n_live;
    if (lane < 3) a.rgb_map[3 * r + lane] = live ? a.rgb_l[3 * slot + lane] : a.rgb0[3 * r + lane];
    if (lane == 0) {
        a.disp_map[r] = live ? a.disp_l[slot] : a.disp0[r];
        a.acc_map[r] = live ? a.acc_l[slot] : a.acc0[r];
        a.depth_map[r] = live ? a.depth_l[slot] : a.depth0[r];
        a.z_std[r] = live ? a.z_std_l[slot] : 0.f;
    }
    const long row = r * a.s_tot, row_l = slot * a.s_tot;
    float4* raw = reinterpret_cast<float4*>(a.raw);
    const float4* raw_l = reinterpret_cast<const float4*>(a.raw_l);
    for (int q = lane; q < a.s_tot; q += kWave) {
        raw[row + q] = live ? raw_l[row_l + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        a.z_vals[row + q] = live ? a.z_vals_l[row_l + q] : 0.f;
    }
    const long srow = r * a.s_fine, srow_l = slot * a.s_fine;
    for (int q = lane; q < a.s_fine; q += kWave) a.z_samples[srow + q] = live ? a.z_samples_l[srow_l + q] : 0.f;
}

}  // namespace

extern "C" int scnerf_ray_compact(const float* acc, float tau, int* live_idx, int* slot_of, int* n_live_dev,
                                  int* n_live_host, long long n, void* stream) {
    SCN_RETURN_IF(n < 0 || n > 0x7fffffffll || !n_live_dev || !(tau >= 0.f && tau < 1.f), SCN_EINVAL);
    SCN_RETURN_IF(n > 0 && (!acc || !live_idx || !slot_of), SCN_EINVAL);
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
    // (n == 0 launches too: the two count words are outputs)
    hipLaunchKernelGGL(ray_compact_kernel, dim3(1), dim3(kCompactThreads), kCompactWaves * sizeof(int), (hipStream_t)stream,
                       acc, tau, live_idx, slot_of, n_live_dev, n_live_host, (long)n);
    return scn_launch_status();
}

extern "C" int scnerf_ray_rows_gather(const float* src, const int* live_idx, float* dst, long long n_live, int w,
                                      long long n_src, void* stream) {
    SCN_RETURN_IF(n_live < 0 || n_src < 0 || n_live > n_src || n_src > 0x7fffffffll || w < 1, SCN_EINVAL);
    if (n_live == 0) return 0;
    SCN_RETURN_IF(!src || !live_idx || !dst, SCN_EINVAL);
    hipLaunchKernelGGL(ray_rows_gather_kernel, dim3(scn_ceil_div(n_live * w, 256)), dim3(256), 0, (hipStream_t)stream,
                       src, live_idx, dst, (long)n_live, w, (long)n_src);
    return scn_launch_status();
}

extern "C" int scnerf_ray_expand(const int* slot_of, long long n, long long n_live, int s_tot, int s_fine,
                                 const float* rgb_l, const float* disp_l, const float* acc_l, const float* depth_l,
                                 const float* z_std_l, const float* raw_l, const float* z_vals_l, const float* z_samples_l,
                                 const float* rgb0, const float* disp0, const float* acc0, const float* depth0,
                                 float* rgb_map, float* disp_map, float* acc_map, float* depth_map, float* z_std, float* raw,
                                 float* z_vals, float* z_samples, void* stream) {
    SCN_RETURN_IF(n < 0 || n > 0x7fffffffll || n_live < 0 || n_live > n || s_tot < 1 || s_fine < 1 || s_fine > s_tot, SCN_EINVAL);
    if (n == 0) return 0;
    SCN_RETURN_IF(!slot_of || !rgb0 || !disp0 || !acc0 || !depth0, SCN_EINVAL);
    SCN_RETURN_IF(!rgb_map || !disp_map || !acc_map || !depth_map || !z_std || !raw || !z_vals || !z_samples, SCN_EINVAL);
    SCN_RETURN_IF(n_live > 0 && (!rgb_l || !disp_l || !acc_l || !depth_l || !z_std_l || !raw_l || !z_vals_l || !z_samples_l),
                  SCN_EINVAL);
    // raw rows move as 16-byte vectors
    SCN_RETURN_IF((reinterpret_cast<unsigned long long>(raw) | reinterpret_cast<unsigned long long>(raw_l)) & 15ull, SCN_EINVAL);
    ExpandArgs a{slot_of, rgb_l, disp_l, acc_l, depth_l, z_std_l, raw_l, z_vals_l, z_samples_l, rgb0, disp0, acc0, depth0,
                 rgb_map, disp_map, acc_map, depth_map, z_std, raw, z_vals, z_samples, (long)n, (long)n_live, s_tot, s_fine};
    hipLaunchKernelGGL(ray_expand_kernel, dim3(scn_ceil_div(n, kExpandWaves)), dim3(kExpandWaves * kWave), 0,
                       (hipStream_t)stream, a);
    return scn_launch_status();
}
