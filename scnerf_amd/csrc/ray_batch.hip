// ray_batch.hip -- one training batch (which pixels of which images, and their colours) in ONE launch.
//
// The reference draws its batch on the host, every step (NeRF/run_nerf.py): from one image, np.random.choice over all
// H W pixels without replacement (a permutation of all of them for N_rand), a meshgrid and three gathers (:409-478); from
// all images, slices of a host permutation of every ray, two host-to-device copies, a gather with host index arrays and
// np.random.shuffle at every epoch end (:368-407).  Here ray j of the batch is pi(position): pi a keyed bijection on [0, M)
// evaluated independently by every thread, so a fresh permutation costs nothing and needs no memory, the first k values
// are a sample without replacement, and ranks that take different positions of the same permutation get disjoint rays
// without talking to each other.
//
// pi: a balanced Feistel network on 2h bits, h the smallest integer >= 1 with 2^(2h) >= M, x = L 2^h + R, four rounds
// (L, R) -> (R, L ^ F_round(R)).  A Feistel network is a bijection whatever F is; with a pseudo-random F four rounds give a
// strong pseudo-random permutation (Luby & Rackoff 1988).  F is Philox4x32-10 (philox.h, the generator of randoms.hip)
// keyed by the seed, counter = (R, tag | mode | round, step or epoch), truncated to h bits.  Values >= M are walked on
// (Black & Rogaway 2002, "cycle walking"): pi restricted to [0, M) by following the cycle until it re-enters.
//
// No atomics, no LDS, nothing read back; the result does not depend on the launch geometry.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "philox.h"
#include "scnerf_hip.h"

namespace {

typedef unsigned long long u64;

constexpr unsigned kTag = 0x52420000u;      // "RB": keeps these counters apart from every other use of the seed
constexpr int kBlock = 64;                  // one wave per workgroup: a batch of a few thousand rays spreads over the CUs

struct Perm {
    u64 m;                                  // the permutation is on [0, m)
    u64 walk_limit;                         // 2^(2h) - m + 1
    unsigned h, mask;                       // half width in bits, 2^h - 1
    unsigned k0, k1;                        // the seed
    unsigned tag;                           // kTag | mode << 8
};

struct Batch {
    Perm p;
    int mode;
    u64 counter;                            // mode 0: the step
    u64 pos0;                               // mode 0: rank n; mode 1: step world n + rank n
    const void* images;
    int image_u8, channels, n_images;
    long long H, W;                         // 64-bit: a 1 x M strip is a legal image, and M goes up to 2^40
    const long long* image_ids;
    long long x0, y0, win_w;
    int image_pos, white_bkgd;
    long long n;
    long long* coords;
    long long* select_inds;
    long long* image_idx;
    float* target;
};

__host__ __device__ inline u64 feistel(const Perm& p, u64 x, unsigned c_lo, unsigned c_hi) {
    unsigned l = (unsigned)(x >> p.h), r = (unsigned)x & p.mask;
#pragma unroll
    for (unsigned round = 0; round < 4; ++round) {
        const unsigned f = scn::philox4x32_10(scn::U4{r, p.tag | round, c_lo, c_hi}, p.k0, p.k1).x & p.mask;
        const unsigned t = l ^ f;
        l = r;
        r = t;
    }
    return ((u64)l << p.h) | r;
}

// pi(x) for x in [0, m).  The walk x, f(x), f(f(x)), ... follows x's cycle of the bijection f on [0, 2^(2h)).  The cycle
// returns to x, which is in range, so an in-range value comes up; until it does the values are pairwise distinct (a
// repeat before the cycle closes would give one value two predecessors) and all lie in [m, 2^(2h)), of which there are
// 2^(2h) - m.  Hence at most 2^(2h) - m + 1 applications: the loop's limit.  2^(2h) < 4 m, so fewer than 4 are expected.
__host__ __device__ inline u64 permute(const Perm& p, u64 x, u64 counter) {
    const unsigned c_lo = (unsigned)counter, c_hi = (unsigned)(counter >> 32);
    u64 v = x;
    for (u64 i = 0; i < p.walk_limit; ++i) {
        v = feistel(p, v, c_lo, c_hi);
        if (v < p.m) return v;
    }
    return x;                               // not reached (see above); in range whatever happens
}

__device__ inline float from_u8(unsigned char v) { return (float)((double)v / 255.0); }   // numpy's fp64 quotient, rounded once

__global__ __launch_bounds__(kBlock) void ray_batch_kernel(Batch b) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.n) return;
    u64 pos = b.pos0 + (u64)j, counter = b.counter;
    if (b.mode == 1) {
        counter = pos / b.p.m;
        pos = pos % b.p.m;
    }
    const u64 index = permute(b.p, pos, counter);
    long long image, y, x;
    if (b.mode == 1) {
        const u64 hw = (u64)b.H * (u64)b.W, rem = index % hw;
        image = (long long)(index / hw);
        y = (long long)(rem / (u64)b.W);
        x = (long long)(rem % (u64)b.W);
    } else {
        image = b.image_pos;
        y = b.y0 + (long long)(index / (u64)b.win_w);
        x = b.x0 + (long long)(index % (u64)b.win_w);
    }
    if (b.coords) {
        b.coords[2 * j] = x;
        b.coords[2 * j + 1] = y;
    }
    if (b.select_inds) b.select_inds[j] = y * b.W + x;
    if (b.image_idx) b.image_idx[j] = image;
    if (b.target) {
        float* t = b.target + 3 * j;
        const long long row = b.image_ids ? b.image_ids[image] : image;
        if (row < 0 || row >= b.n_images) {             // a bad entry of image_ids: nothing is read
            t[0] = t[1] = t[2] = __uint_as_float(0x7fc00000u);
            return;
        }
        const long long pixel = (row * b.H + y) * b.W + x;
        if (!b.image_u8) {
            const float* s = (const float*)b.images + 3 * pixel;
            t[0] = s[0]; t[1] = s[1]; t[2] = s[2];
        } else {
            const unsigned char* s = (const unsigned char*)b.images + b.channels * pixel;
            const float r = from_u8(s[0]), g = from_u8(s[1]), bl = from_u8(s[2]);
            if (b.channels == 4 && b.white_bkgd) {
                const float a = from_u8(s[3]), rest = 1.f - a;
                t[0] = r * a + rest; t[1] = g * a + rest; t[2] = bl * a + rest;
            } else {
                t[0] = r; t[1] = g; t[2] = bl;
            }
        }
    }
}

}  // namespace

extern "C" int scnerf_ray_batch(int mode, unsigned long long seed, unsigned long long step, const void* images, int image_u8,
                                int channels, int n_images, long long H, long long W, const int64_t* image_ids, int n_sel,
                                int image_pos, long long win_x0, long long win_y0, long long win_w, long long win_h,
                                long long n, int rank, int world, int white_bkgd, int64_t* coords, int64_t* select_inds,
                                int64_t* image_idx, float* target, void* stream) {
    SCN_RETURN_IF(mode != 0 && mode != 1, SCN_EINVAL);
    SCN_RETURN_IF(n < 0 || H < 1 || W < 1 || n_sel < 1 || n_images < 1 || world < 1 || rank < 0 || rank >= world, SCN_EINVAL);
    SCN_RETURN_IF(image_ids == nullptr && n_sel > n_images, SCN_EINVAL);
    const u64 limit = 1ull << 40;                                   // rays of an image, and of the permutation
    SCN_RETURN_IF((u64)H >= limit || (u64)W >= limit || (u64)H > (limit - 1) / (u64)W, SCN_EINVAL);
    SCN_RETURN_IF(win_w < 1 || win_h < 1 || win_x0 < 0 || win_y0 < 0 || win_x0 > W || win_y0 > H || win_w > W - win_x0 ||
                  win_h > H - win_y0, SCN_EINVAL);
    SCN_RETURN_IF(target != nullptr && images == nullptr, SCN_EINVAL);
    SCN_RETURN_IF(images != nullptr && (image_u8 ? (channels != 3 && channels != 4) : channels != 3), SCN_EINVAL);
    u64 m;
    if (mode == 1) {
        SCN_RETURN_IF(win_x0 != 0 || win_y0 != 0 || win_w != W || win_h != H, SCN_EINVAL);
        const u64 hw = (u64)H * (u64)W;
        SCN_RETURN_IF((u64)n_sel > (limit - 1) / hw, SCN_EINVAL);
        m = (u64)n_sel * hw;
    } else {
        SCN_RETURN_IF(image_pos < 0 || image_pos >= n_sel, SCN_EINVAL);
        m = (u64)win_w * (u64)win_h;                                // a window inside the image: below the limit
    }
    // positions: all of them below 2^63 (exact in 128 bits, then narrowed)
    const unsigned __int128 per_step = (unsigned __int128)(u64)world * (u64)n;
    SCN_RETURN_IF(per_step >> 63, SCN_EINVAL);
    const unsigned __int128 last = (mode == 1 ? (unsigned __int128)step * per_step : 0) + per_step;
    SCN_RETURN_IF(last >> 63, SCN_EINVAL);
    SCN_RETURN_IF(mode == 0 && per_step > m, SCN_EINVAL);
    if (n == 0) return 0;

    Batch b;
    unsigned h = 1;
    while (h < 20 && (1ull << (2 * h)) < m) ++h;
    b.p.m = m;
    b.p.h = h;
    b.p.mask = (1u << h) - 1u;
    b.p.walk_limit = (1ull << (2 * h)) - m + 1;
    b.p.k0 = (unsigned)seed;
    b.p.k1 = (unsigned)(seed >> 32);
    b.p.tag = kTag | ((unsigned)mode << 8);
    b.mode = mode;
    b.counter = step;
    b.pos0 = (mode == 1 ? (u64)step * (u64)per_step : 0) + (u64)rank * (u64)n;
    b.images = images;
    b.image_u8 = image_u8;
    b.channels = channels;
    b.n_images = n_images;
    b.H = H;
    b.W = W;
    b.image_ids = (const long long*)image_ids;
    b.image_pos = image_pos;
    b.x0 = win_x0;
    b.y0 = win_y0;
    b.win_w = win_w;
    b.white_bkgd = white_bkgd;
    b.n = n;
    b.coords = (long long*)coords;
    b.select_inds = (long long*)select_inds;
    b.image_idx = (long long*)image_idx;
    b.target = target;
    const long long blocks = (n + kBlock - 1) / kBlock;
    SCN_RETURN_IF(blocks > 0x7fffffffLL, SCN_ENOSUP);
    hipLaunchKernelGGL(ray_batch_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, b);
    return scn_launch_status();
}
