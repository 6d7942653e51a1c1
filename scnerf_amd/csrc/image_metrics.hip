// image_metrics.hip -- SSIM, squared error (MSE / PSNR) and optionally the SSIM map of two image batches in ONE pass.
//
// The evaluation half of the reference's loop: img2mse / mse2psnr / piqa.ssim.SSIM per test and train image
// (/root/reference NeRF/run_nerf.py:748-795, :987-1040; nerfplusplus/ddp_test_nerf.py:122-196).  SSIM after Wang et al. 2004
// with the defaults piqa documents: a separable Gaussian window (11 taps, sigma 1.5), no padding, channel-wise; see
// INTEGRATION.md for the definition this file transcribes.
//
// One 256-thread workgroup owns, for one (image, channel), a 32 x 32 block of window origins -- and the same 32 x 32 block of
// PIXELS for the squared error, so every pixel is counted once, the last win-1 rows and columns (which start no window) too:
//   1. stage the (32 + win - 1)^2 halo tiles of x and y in LDS (raw values, zero outside the image);
//   2. squared error of the owned pixels (x NOT clamped: run_nerf.py:757-759 scores the unclipped render);
//   3. horizontal pass: five maps g*x, g*y, g*(x x), g*(y y), g*(x y) of (32 + win - 1) rows x 32 columns into LDS,
//      x clamped to [0, L] here when clip_x is set (run_nerf.py:763-771 clips what SSIM sees);
//   4. vertical pass in registers (four origins of one column per thread), the SSIM expression op by op in fp32;
//   5. everything beyond one pixel's value is summed in fp64: per thread, per wave (shuffles), per workgroup (LDS).
// The workgroup writes its two partial sums to ITS slot of the workspace; a second launch adds an image's slots in a fixed
// order.  No floating-point atomics: results are bit-identical from call to call, and an image's result does not depend on
// what else is in the batch.
//
// LDS: 2 x 42 x 43 + 5 x 42 x 33 floats = 42 168 bytes.  Row strides are odd (43, 33): with ds_read_b32 / ds_write_b32 banking
// (address / 4 mod 32 within a 32-lane half, cdna_hip_programming.md section 2 and Guideline 4) the horizontal pass -- a half-wave
// covers 4 rows x 8 column groups of 4 -- reads banks 11 r + 4 g + i and writes banks r + 4 g + o, all distinct; the staging, the
// squared error and the vertical pass walk rows with consecutive lanes.
//
// Global loads: a wave walks one tile row.  For a unit-stride row (NCHW) lane k reads column k.  For channel-last memory (the
// .permute(2, 0, 1)[None] view of an [H, W, C] image, run_nerf.py:767) lane k reads float k of the INTERLEAVED row -- consecutive
// lanes, consecutive addresses -- and the lanes holding this workgroup's channel deposit theirs.  Any other strides: lane k reads
// column k at its stride.
#include <scn_wave.h>

#include "launch.h"
#include "scnerf_hip.h"

namespace {

using namespace scn;

constexpr int kTile = 32;                          // window origins (and owned pixels) per tile edge
constexpr int kMinWin = 3, kMaxWin = 11;
constexpr int kHalo = kTile + kMaxWin - 1;         // 42
constexpr int kStageStride = kHalo + 1;            // 43
constexpr int kMapStride = kTile + 1;              // 33
constexpr int kStageFloats = kHalo * kStageStride;
constexpr int kMapFloats = kHalo * kMapStride;
constexpr int kLdsBytes = (2 * kStageFloats + 5 * kMapFloats) * 4;
constexpr int kMaxInterleave = 64;                 // channel counts the interleaved-row loader takes (else: strided columns)
constexpr int kSlotDoubles = 2;                    // per workgroup: {sum of ss, sum of squared differences}

struct Image {
    const float* p;
    long long sn, sc, sh, sw;                      // element strides
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor(v, o);
    return v;
}

// The halo tile of channel `c` of image `n` at pixel (y0, x0) into s[halo rows][kStageStride], zero outside the image.
__device__ __forceinline__ void stage_tile(float* s, const Image im, int n, int c, int nchan, int y0, int x0, int h, int w,
                                           int halo) {
    // interleaved row: floats [x0 C, (x0 + halo) C) are consecutive; float k is column k / C, channel k mod C
    const bool interleaved = im.sc == 1 && im.sw == nchan && nchan > 1 && nchan <= kMaxInterleave;
    const int group = interleaved ? nchan : 1;
    const int chan = interleaved ? c : 0;
    const long long step = interleaved ? 1 : im.sw;
    // k / group for k < halo * group as a multiply and a shift (exact while k * group < 2^24)
    const unsigned magic = (1u << 24) / (unsigned)group + 1u;
    const float* base = im.p + (long long)n * im.sn + (long long)x0 * im.sw + (interleaved ? 0 : (long long)c * im.sc);
    const int lane = lane_id();
    for (int r = wave_id(); r < halo; r += 4) {
        const bool row_in = y0 + r < h;
        const float* row = base + (long long)(y0 + r) * im.sh;
        for (int k = lane; k < halo * group; k += kWave) {
            const int col = (int)(((unsigned)k * magic) >> 24);
            const int ch = k - col * group;
            float v = 0.f;
            if (row_in && x0 + col < w) v = row[(long long)k * step];
            if (ch == chan) s[r * kStageStride + col] = v;
        }
    }
}

template <int WIN>
__global__ __launch_bounds__(256) void image_metrics_kernel(const Image x, const Image y, int nchan, int h, int w,
                                                            const float* __restrict__ taps, float c1, float c2,
                                                            float value_range, int clip_x, float* __restrict__ map_out,
                                                            double* __restrict__ slots, int tiles_x, int tiles_y) {
    constexpr int kNeed = kTile + WIN - 1;          // halo rows / columns this window size uses
    float* xs = dynamic_lds<float>();
    float* ys = xs + kStageFloats;
    float* hm = ys + kStageFloats;                  // five maps [kNeed rows][kMapStride]

    const int tid = (int)threadIdx.x;
    int b = (int)blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int nc = b / tiles_y;
    const int n = nc / nchan, c = nc - n * nchan;
    const int x0 = tx * kTile, y0 = ty * kTile;
    const int ow = w - WIN + 1, oh = h - WIN + 1;   // extents of the map

    stage_tile(xs, x, n, c, nchan, y0, x0, h, w, kNeed);
    stage_tile(ys, y, n, c, nchan, y0, x0, h, w, kNeed);
    block_sync();

    // squared error of the pixels this tile owns
    double sse = 0.0;
    {
        const int col = tid & 31;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (tid >> 5) + 8 * i;
            if (y0 + r < h && x0 + col < w) {
                const float d = xs[r * kStageStride + col] - ys[r * kStageStride + col];
                sse += (double)(d * d);
            }
        }
    }

    double ssum = 0.0;
    if (x0 < ow && y0 < oh) {                       // the tile starts at least one window (the same for the whole workgroup)
        float g[WIN];
#pragma unroll
        for (int t = 0; t < WIN; ++t) g[t] = taps[t];

        // horizontal pass: (row, group of four columns) per thread
        for (int item = tid; item < kNeed * 8; item += 256) {
            const int r = item >> 3, q = (item & 7) * 4;
            float a[WIN + 3], bb[WIN + 3], aa[WIN + 3], bq[WIN + 3], ab[WIN + 3];
#pragma unroll
            for (int i = 0; i < WIN + 3; ++i) {
                float xv = xs[r * kStageStride + q + i];
                const float yv = ys[r * kStageStride + q + i];
                if (clip_x) xv = xv < 0.f ? 0.f : (xv > value_range ? value_range : xv);    // (a NaN stays a NaN)
                a[i] = xv;
                bb[i] = yv;
                aa[i] = xv * xv;
                bq[i] = yv * yv;
                ab[i] = xv * yv;
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
                for (int t = 0; t < WIN; ++t) {
                    m0 = fmaf(g[t], a[o + t], m0);
                    m1 = fmaf(g[t], bb[o + t], m1);
                    m2 = fmaf(g[t], aa[o + t], m2);
                    m3 = fmaf(g[t], bq[o + t], m3);
                    m4 = fmaf(g[t], ab[o + t], m4);
                }
                float* dst = hm + r * kMapStride + q + o;
                dst[0 * kMapFloats] = m0;
                dst[1 * kMapFloats] = m1;
                dst[2 * kMapFloats] = m2;
                dst[3 * kMapFloats] = m3;
                dst[4 * kMapFloats] = m4;
            }
        }
        block_sync();

        // vertical pass: four origins of one column per thread
        const int col = tid & 31, r0 = (tid >> 5) * 4;
        float acc[5][4];
#pragma unroll
        for (int m = 0; m < 5; ++m)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[m][o] = 0.f;
#pragma unroll
        for (int i = 0; i < WIN + 3; ++i) {
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                const float v = hm[m * kMapFloats + (r0 + i) * kMapStride + col];
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (i - o >= 0 && i - o < WIN) acc[m][o] = fmaf(g[i - o], v, acc[m][o]);
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int oy = y0 + r0 + o, ox = x0 + col;
            if (oy < oh && ox < ow) {
                const float mu_x = acc[0][o], mu_y = acc[1][o];
                const float mxx = mu_x * mu_x, myy = mu_y * mu_y, mxy = mu_x * mu_y;
                const float sxx = acc[2][o] - mxx, syy = acc[3][o] - myy, sxy = acc[4][o] - mxy;
                const float cs = (2.f * sxy + c2) / (sxx + syy + c2);
                const float ss = (2.f * mxy + c1) / (mxx + myy + c1) * cs;
                ssum += (double)ss;
                if (map_out) map_out[((long long)nc * oh + oy) * ow + ox] = ss;
            }
        }
    }

    ssum = wave_sum(ssum);
    sse = wave_sum(sse);
    block_sync();                                   // every wave is done with the tiles: the head of the LDS carries the wave sums
    double* red = dynamic_lds<double>();
    if (lane_id() == 0) {
        red[2 * wave_id()] = ssum;
        red[2 * wave_id() + 1] = sse;
    }
    block_sync();
    if (tid == 0) {
        double* slot = slots + (long long)blockIdx.x * kSlotDoubles;
        slot[0] = ((red[0] + red[2]) + red[4]) + red[6];
        slot[1] = ((red[1] + red[3]) + red[5]) + red[7];
    }
}

// One wave per image: its slots in a fixed order, then the two means as fp32.
__global__ __launch_bounds__(64) void image_metrics_finish_kernel(const double* __restrict__ slots, int per_image,
                                                                  double map_count, double pixel_count,
                                                                  float* __restrict__ ssim_out, float* __restrict__ mse_out) {
    const int n = (int)blockIdx.x, lane = lane_id();
    const double* s = slots + (long long)n * per_image * kSlotDoubles;
    double ssum = 0.0, sse = 0.0;
    for (int i = lane; i < per_image; i += kWave) {
        ssum += s[(long long)i * kSlotDoubles];
        sse += s[(long long)i * kSlotDoubles + 1];
    }
    ssum = wave_sum(ssum);
    sse = wave_sum(sse);
    if (lane == 0) {
        ssim_out[n] = (float)(ssum / map_count);
        mse_out[n] = (float)(sse / pixel_count);
    }
}

long long tile_count(int n, int c, int h, int w) {
    return (long long)n * c * ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
}

template <int WIN>
void launch_metrics(long long blocks, hipStream_t stream, const Image& x, const Image& y, int c, int h, int w,
                    const float* taps, float c1, float c2, float value_range, int clip_x, float* map_out, double* slots,
                    int tiles_x, int tiles_y) {
    hipLaunchKernelGGL(image_metrics_kernel<WIN>, dim3((unsigned)blocks), dim3(256), kLdsBytes, stream, x, y, c, h, w, taps,
                       c1, c2, value_range, clip_x, map_out, slots, tiles_x, tiles_y);
}

}  // namespace

extern "C" long long scnerf_image_metrics_workspace_floats(int n, int c, int h, int w, int win) {
    (void)win;                                      // the tiling does not depend on the window
    if (n < 0 || c < 0 || h < 0 || w < 0) return 0;
    return tile_count(n, c, h, w) * kSlotDoubles * 2;
}

extern "C" int scnerf_image_metrics(const float* x, long long x_sn, long long x_sc, long long x_sh, long long x_sw,
                                    const float* y, long long y_sn, long long y_sc, long long y_sh, long long y_sw, int n,
                                    int c, int h, int w, const float* taps, int win, float c1, float c2, float value_range,
                                    int clip_x, float* ssim_out, float* mse_out, float* map_out, float* workspace,
                                    void* stream) {
    SCN_RETURN_IF(n < 0 || c < 1 || win < kMinWin || win > kMaxWin || (win & 1) == 0, SCN_EINVAL);
    if (n == 0) return 0;
    SCN_RETURN_IF(!x || !y || !taps || !ssim_out || !mse_out || !workspace, SCN_EINVAL);
    SCN_RETURN_IF(h < win || w < win, SCN_EINVAL);
    SCN_RETURN_IF((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0, SCN_EINVAL);      // the slots are doubles
    const long long blocks = tile_count(n, c, h, w);
    SCN_RETURN_IF(blocks > 0x7fffffffLL || (long long)n * c > 0x7fffffffLL, SCN_ENOSUP);
    const int tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    const Image xi = {x, x_sn, x_sc, x_sh, x_sw}, yi = {y, y_sn, y_sc, y_sh, y_sw};
    double* slots = reinterpret_cast<double*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    switch (win) {
        case 3: launch_metrics<3>(blocks, s, xi, yi, c, h, w, taps, c1, c2, value_range, clip_x, map_out, slots, tiles_x, tiles_y); break;
        case 5: launch_metrics<5>(blocks, s, xi, yi, c, h, w, taps, c1, c2, value_range, clip_x, map_out, slots, tiles_x, tiles_y); break;
        case 7: launch_metrics<7>(blocks, s, xi, yi, c, h, w, taps, c1, c2, value_range, clip_x, map_out, slots, tiles_x, tiles_y); break;
        case 9: launch_metrics<9>(blocks, s, xi, yi, c, h, w, taps, c1, c2, value_range, clip_x, map_out, slots, tiles_x, tiles_y); break;
        default: launch_metrics<11>(blocks, s, xi, yi, c, h, w, taps, c1, c2, value_range, clip_x, map_out, slots, tiles_x, tiles_y); break;
    }
    const int status = scn_launch_status();
    if (status != 0) return status;
    const double map_count = (double)c * (double)(h - win + 1) * (double)(w - win + 1);
    const double pixel_count = (double)c * (double)h * (double)w;
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3((unsigned)n), dim3(64), 0, s, (const double*)slots,
                       (int)(blocks / n), map_count, pixel_count, ssim_out, mse_out);
    return scn_launch_status();
}
