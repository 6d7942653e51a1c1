// wgrad.hip -- weight / bias gradients of one linear layer as an fp32-MFMA GEMM reduced over the
// samples:  dW[n][k] = sum_p dZ[p][n] * X[p][k],  db[n] = sum_p dZ[p][n]   (+ an optional rank-1
// side product  dv[k] = sum_p v[p] * X[p][k]  used for alpha_linear, whose single output row
// would waste a whole MFMA tile).
//
// What autograd derives for every nn.Linear of the reference network
// (NeRF/run_nerf_helpers.py:13-21, :105-128).
//
// dZ and X are the row-major [P][ld] tensors left in HBM by mlp_bwd.hip / the training forward,
// so both MFMA operands are 128-byte row segments: lane l supplies A[i = l&31][k = l>>5] =
// dZ[p = 2s + (l>>5)][n0 + (l&31)] and B likewise from X.  A workgroup (4 waves, 2 x 2) owns the
// whole [BN x BK] output for a contiguous chunk of samples, staging 16 samples at a time through
// double-buffered LDS; partial results go to a workspace and a second kernel reduces them in a
// fixed order (deterministic; 64 MB per 256x256 layer at 256 chunks is ~25 us of HBM time).
//
// The file is kernels first (the generic GEMM, vecmat, rows4, the reductions, the lean group's finishing kernel; the
// 256 x 256, tiles and fp16 kernels are in their own headers), then the host side:
//   launchers      one per kernel family: opt into the LDS size, launch, report the status
//   descriptors    Operand / Target / Samples: what a GEMM reads, where its sums go, how the samples are cut
//                  (chunk_samples is the one chunk rule);  Partials hands out the [G][BN][BK] (+ [G][BN]) slabs of a
//                  workspace and fails the call rather than cross its limit;  reduce_job fills a ReduceJob, ReduceQueue
//                  collects up to kMaxJobs of them for the merged reduction
//   single_gemm    one GEMM with the kernel picked at run time from the operands: scnerf_wgrad and
//                  scnerf_wgrad_half_narrow, through which the tests reach each kernel family on its own
//   nerf_wgrad<PD> a network pass: it names the launch every gradient takes (Var<PD>::kEW fixes the narrow shapes) and
//                  lays its slabs out below the lean group's scratch;  the three scnerf_nerf_wgrad* exports share
//                  one body, nerf_wgrad_entry
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include <scn_wave.h>

#include "launch.h"
#include "mlp_common.h"
#include "mlp_h3.h"
#include "scnerf_hip.h"
#include "wgrad256.h"
#include "wgrad256_half.h"
#include "wgrad_half_narrow.h"
#include "wgrad_tiles.h"

namespace {

using namespace scn;

constexpr int kThreads = 256;
constexpr int kMS = 32;   // samples per LDS stage = one wave tile of the MLP kernels

struct WgradArgs {
    const float* A; int lda; int n_load; int a_tiled;   // dZ: tile-native section of width lda, or row-major [P][lda]
    const float* B; int ldb; int k_load; int b_tiled;   // X : likewise
    long P;                                             // valid samples (row-major operands are masked beyond)
    long Ppad;                                          // samples the tile-native sections cover
    long chunk;                                         // samples per workgroup (multiple of kMS)
    float* part_w;                                      // [G][BN][BK]
    float* part_b;                                      // [G][BN]
};

// LDS image of one staged operand: row-major [kMS samples][width + 4] (the 4-float pad makes the
// 16-byte writes of 8 consecutive samples and the 4-byte reads of 32 consecutive columns both
// conflict-free).  A 16-byte piece of either HBM layout holds 4 consecutive columns of one sample:
//   row-major source : piece e -> sample e / width, column e % width
//   tile-native source: piece index e/4 = (t*4 + q)*64 + lane, lane = m + 32 h -> sample m,
//                       column 32 t + 8 q + 4 h
__device__ __forceinline__ int lds_piece_offset(int e, int width, int tiled) {
    int m, c;
    if (tiled) {
        const int piece = e >> 2, ln = piece & 63, tq = piece >> 6;
        m = ln & 31;
        c = (tq >> 2) * 32 + (tq & 3) * 8 + (ln >> 5) * 4;
    } else {
        m = e / width;
        c = e % width;
    }
    return m * (width + 4) + c;
}

// FAST: both operands tile-native -- every staged piece exists (the sections are padded), so the loads are
// unconditional; otherwise rows beyond P / columns beyond n_load of a row-major operand read as zero.
template <int WN, int WK, bool FAST>
__global__ __launch_bounds__(kThreads, 1) void wgrad_kernel(WgradArgs a) {
    constexpr int BN = 2 * WN * 32, BK = 2 * WK * 32;
    constexpr int LDA = BN + 4, LDB = BK + 4;              // padded LDS row strides
    constexpr int STAGE = kMS * (LDA + LDB);               // floats per LDS stage
    constexpr int A_F4 = kMS * BN / 4 / kThreads, B_F4 = kMS * BK / 4 / kThreads;
    static_assert(kMS * BN % (4 * kThreads) == 0 && kMS * BK % (4 * kThreads) == 0, "stage shape");
    float* lds = dynamic_lds<float>();
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const int wn = wave >> 1, wk = wave & 1;
    const int wk_uniform = uniform(wk);
    const int li = lane & 31, mh = lane >> 5;
    const long p_begin = (long)blockIdx.x * a.chunk;
    const long p_lim = a.Ppad;                              // tiles exist up to here
    const long p_end = min(p_lim, p_begin + a.chunk);
    const int n_stage = p_begin < p_end ? (int)((p_end - p_begin + kMS - 1) / kMS) : 0;

    f32x16 acc[WN][WK];
#pragma unroll
    for (int i = 0; i < WN; ++i)
#pragma unroll
        for (int j = 0; j < WK; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float bsum[WN];
#pragma unroll
    for (int i = 0; i < WN; ++i) bsum[i] = 0.f;

    int a_dst[A_F4], b_dst[B_F4];      // where this thread's staged pieces go in the LDS image
#pragma unroll
    for (int q = 0; q < A_F4; ++q) a_dst[q] = lds_piece_offset((q * kThreads + tid) * 4, BN, a.a_tiled);
#pragma unroll
    for (int q = 0; q < B_F4; ++q) b_dst[q] = lds_piece_offset((q * kThreads + tid) * 4, BK, a.b_tiled);

    // per-thread source offsets of the staged 16-byte pieces, relative to the stage's first sample
    // (computed once: the address arithmetic must not sit in front of every stage's MFMAs)
    int a_src[A_F4], b_src[B_F4], a_row[A_F4], b_row[B_F4];
#pragma unroll
    for (int q = 0; q < A_F4; ++q) {
        const int e = (q * kThreads + tid) * 4;
        if (a.a_tiled) { a_src[q] = e; a_row[q] = 0; }
        else { a_src[q] = (e / BN) * a.lda + e % BN; a_row[q] = (e % BN) < a.n_load ? e / BN : kMS; }
    }
#pragma unroll
    for (int q = 0; q < B_F4; ++q) {
        const int e = (q * kThreads + tid) * 4;
        if (a.b_tiled) { b_src[q] = e; b_row[q] = 0; }
        else { b_src[q] = (e / BK) * a.ldb + e % BK; b_row[q] = (e % BK) < a.k_load ? e / BK : kMS; }
    }
    f32x4 sa[A_F4], sb[B_F4];
    auto issue = [&](int st) {
        const long p0 = p_begin + (long)st * kMS;
        // tile-native: the 32-sample block starts at p0 * ld; row-major: row p0.  Rows >= P of a
        // row-major operand are zero (tile-native sections hold zeros / finite values there).
        const float* As0 = a.A + p0 * a.lda;
        const float* Bs0 = a.B + p0 * a.ldb;
        const int rows = (int)min((long)kMS, a.P - p0);       // valid rows of a row-major operand
        const int rows_a = a.a_tiled ? kMS : rows, rows_b = a.b_tiled ? kMS : rows;
        if constexpr (FAST) {
#pragma unroll
            for (int q = 0; q < A_F4; ++q) sa[q] = *reinterpret_cast<const f32x4*>(As0 + (q * kThreads + tid) * 4);
#pragma unroll
            for (int q = 0; q < B_F4; ++q) sb[q] = *reinterpret_cast<const f32x4*>(Bs0 + (q * kThreads + tid) * 4);
        } else {
#pragma unroll
            for (int q = 0; q < A_F4; ++q) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (a_row[q] < rows_a) v = *reinterpret_cast<const f32x4*>(As0 + a_src[q]);
                sa[q] = v;
            }
#pragma unroll
            for (int q = 0; q < B_F4; ++q) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (b_row[q] < rows_b) v = *reinterpret_cast<const f32x4*>(Bs0 + b_src[q]);
                sb[q] = v;
            }
        }
    };
    auto commit = [&](int buf) {
        float* s = lds + buf * STAGE;
#pragma unroll
        for (int q = 0; q < A_F4; ++q) *reinterpret_cast<f32x4*>(s + a_dst[q]) = sa[q];
#pragma unroll
        for (int q = 0; q < B_F4; ++q) *reinterpret_cast<f32x4*>(s + kMS * LDA + b_dst[q]) = sb[q];
    };

    if (n_stage > 0) {
        issue(0);
        commit(0);
    }
    block_sync();
    // (unrolling the stage loop by two to make `buf` a compile-time constant spills: 632 B/lane of scratch)
    for (int st = 0; st < n_stage; ++st) {
        const int buf = st & 1;
        const bool more = st + 1 < n_stage;
        if (more) issue(st + 1);
        sched_fence();          // the global loads stay at the head of the stage
        const float* As = lds + buf * STAGE;
        const float* Bs = As + kMS * LDA;
        // operands of step s+1 are read while the WN x WK MFMAs of step s run
        float av[2][WN], bv[2][WK];
        auto read_step = [&](int s2, int slot) {
            const int m = 2 * s2 + mh;
#pragma unroll
            for (int i = 0; i < WN; ++i) av[slot][i] = As[m * LDA + (wn * WN + i) * 32 + li];
#pragma unroll
            for (int j = 0; j < WK; ++j) bv[slot][j] = Bs[m * LDB + (wk * WK + j) * 32 + li];
        };
        read_step(0, 0);
#pragma unroll
        for (int s = 0; s < kMS / 2; ++s) {
            const int cur = s & 1;
            if (s + 1 < kMS / 2) read_step(s + 1, cur ^ 1);
            if (s == (kMS / 2) * 3 / 4 && more) commit(buf ^ 1);
            sched_fence();
#pragma unroll
            for (int i = 0; i < WN; ++i)
#pragma unroll
                for (int j = 0; j < WK; ++j) acc[i][j] = mfma_32x32x2(av[cur][i], bv[cur][j], acc[i][j]);
            if (wk_uniform == 0) {       // wave-uniform: a real branch, not 2 x WN selects for every wave
#pragma unroll
                for (int i = 0; i < WN; ++i) bsum[i] += av[cur][i];
            }
        }
        block_sync();
    }

    // ---- partial results -----------------------------------------------------------------
    float* pw = a.part_w + (long)blockIdx.x * BN * BK;
#pragma unroll
    for (int i = 0; i < WN; ++i)
#pragma unroll
        for (int j = 0; j < WK; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = (wn * WN + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * mh;
                const int k = (wk * WK + j) * 32 + li;
                pw[n * BK + k] = acc[i][j][r];
            }
    if (wk == 0) {
#pragma unroll
        for (int i = 0; i < WN; ++i) {
            const float tot = bsum[i] + shfl_xor(bsum[i], 32);
            if (mh == 0) a.part_b[(long)blockIdx.x * BN + (wn * WN + i) * 32 + li] = tot;
        }
    }
}

// dv[k] = sum_p v[p] * X[p][k] for a tile-native X of width 256 (alpha_linear's weight gradient:
// v = d sigma, X = the last trunk activation), and sum_p v[p] (its bias gradient).  HBM-bound: X is
// read once.  Thread `tid` owns the 16-byte pieces tid + 256 i (i < 8) of every tile it visits, i.e.
// always the same 4 features of the same in-tile sample, so it accumulates them privately; the 32
// samples of a tile are then folded with shuffles and the workgroups' partials are summed in a fixed
// order by wgrad_reduce_kernel.
__global__ __launch_bounds__(kThreads) void vecmat_kernel(const float* __restrict__ X, const float* __restrict__ vec,
                                                          int vec_stride, long P, long n_tiles,
                                                          float* __restrict__ part /* [G][257] */) {
    const int tid = threadIdx.x, lane = lane_id();
    const int m = lane & 31;
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float vs = 0.f;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long p = tile * 32 + m;
        const float v = p < P ? vec[p * vec_stride] : 0.f;
        if (tid < 32) vs += v;
        const f32x4* blk = reinterpret_cast<const f32x4*>(X + tile * (32L * 256));
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 x = blk[tid + kThreads * i];
            acc[i][0] = fmaf(v, x[0], acc[i][0]); acc[i][1] = fmaf(v, x[1], acc[i][1]);
            acc[i][2] = fmaf(v, x[2], acc[i][2]); acc[i][3] = fmaf(v, x[3], acc[i][3]);
        }
    }
    // fold the 32 samples (lanes with equal lane >> 5); piece tid + 256 i = (t*4+q)*64 + lane
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = acc[i][j];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) x += shfl_xor(x, o);
            acc[i][j] = x;
        }
    float vt = vs;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) vt += shfl_xor(vt, o);
    float* out = part + (long)blockIdx.x * 257;
    if (m == 0) {
        const int h = lane >> 5;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int tq = ((tid + kThreads * i) >> 6);        // t*4 + q
            const int c = (tq >> 2) * 32 + (tq & 3) * 8 + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[c + j] = acc[i][j];
        }
        if (tid == 0) out[256] = vt;
    }
}

// dW[c][k] = sum_p V[p][c] * X[p][k], db[c] = sum_p V[p][c] for c < 4: V row-major [P][4], X tile-native of width 128
// (rgb_linear's weight gradient: V = d_raw, whose fourth column -- d sigma -- is summed along and not reduced; X = the
// hidden layer of the views branch).  As vecmat_kernel: HBM-bound, X is read once, a thread owns the same 4 features of
// the same in-tile sample in every tile it visits; two tiles per iteration keep eight 16-byte loads in flight per thread.
// Partials [G][4][128] and [G][4] in ReduceJob's layout.
__global__ __launch_bounds__(kThreads) void rows4_kernel(const float* __restrict__ X, const float* __restrict__ V, long P,
                                                         long n_tiles, float* __restrict__ part_w, float* __restrict__ part_b) {
    const int tid = threadIdx.x, lane = lane_id();
    const int m = lane & 31;
    f32x4 acc[4][4];       // [piece][row]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 vs = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long tile = blockIdx.x; tile < n_tiles; tile += 2L * gridDim.x) {
        const long tile2 = tile + gridDim.x;
        const bool two = tile2 < n_tiles;
        const long p0 = tile * 32 + m, p1 = tile2 * 32 + m;
        const f32x4 v0 = p0 < P ? *reinterpret_cast<const f32x4*>(V + p0 * 4) : zero;
        const f32x4 v1 = (two && p1 < P) ? *reinterpret_cast<const f32x4*>(V + p1 * 4) : zero;
        if (tid < 32) vs += v0 + v1;
        const f32x4* blk0 = reinterpret_cast<const f32x4*>(X + tile * (32L * 128));
        const f32x4* blk1 = reinterpret_cast<const f32x4*>(X + (two ? tile2 : tile) * (32L * 128));
        f32x4 x0[4], x1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { x0[i] = blk0[tid + kThreads * i]; x1[i] = blk1[tid + kThreads * i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][c][j] = fmaf(v1[c], x1[i][j], fmaf(v0[c], x0[i][j], acc[i][c][j]));
    }
    // fold the 32 samples (lanes with equal lane >> 5); piece tid + 256 i = (t * 4 + q) * 64 + lane
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = acc[i][c][j];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) x += shfl_xor(x, o);
                acc[i][c][j] = x;
            }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float x = vs[c];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) x += shfl_xor(x, o);
        vs[c] = x;
    }
    float* ow = part_w + (long)blockIdx.x * (4 * 128);
    if (m == 0) {
        const int h = lane >> 5;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tq = (tid + kThreads * i) >> 6;          // t * 4 + q
            const int col = (tq >> 2) * 32 + (tq & 3) * 8 + 4 * h;
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(ow + c * 128 + col) = acc[i][c];
        }
        if (tid == 0) *reinterpret_cast<f32x4*>(part_b + (long)blockIdx.x * 4) = vs;
    }
}

// fixed-order sum over the G partials with four independent accumulators (four loads in flight per
// thread: the single-accumulator loop was latency-bound at ~1 TB/s)
__device__ __forceinline__ float sum_partials(const float* __restrict__ p, long stride, int G) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 3 < G; g += 4) {
        const float a = p[(long)g * stride], b = p[(long)(g + 1) * stride];
        const float c = p[(long)(g + 2) * stride], d = p[(long)(g + 3) * stride];
        s0 += a; s1 += b; s2 += c; s3 += d;
    }
    for (; g < G; ++g) s0 += p[(long)g * stride];
    return (s0 + s1) + (s2 + s3);
}

// out[n * ldo + col0 + k] = sum_g part[g][n][k]   (n < n_out, k < k_out), fixed order over g
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(
    const float* __restrict__ part_w, const float* __restrict__ part_b, int G, int BN, int BK, int n_out,
    int k_out, float* __restrict__ dW, int ldo, int col0, float* __restrict__ db) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nw = (long)n_out * k_out;
    if (idx < nw) {
        const int n = (int)(idx / k_out), k = (int)(idx % k_out);
        dW[(long)n * ldo + col0 + k] = sum_partials(part_w + (long)n * BK + k, (long)BN * BK, G);
        return;
    }
    const long j = idx - nw;
    if (db && j < n_out) db[j] = sum_partials(part_b + j, BN, G);
}

// dv[k] (+)= sum_g part[g][k] (k < 256), *dvsum (+)= sum_g part[g][256]
__global__ __launch_bounds__(256) void vecmat_reduce_kernel(const float* __restrict__ part, int G,
                                                            float* __restrict__ dv, float* __restrict__ dvsum,
                                                            int accumulate) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < 256) {
        const float v = sum_partials(part + k, 257, G);
        dv[k] = accumulate ? dv[k] + v : v;
    } else if (k == 256 && dvsum) {
        const float v = sum_partials(part + 256, 257, G);
        *dvsum = accumulate ? *dvsum + v : v;
    }
}

// ---- all reductions of one network pass in ONE launch -----------------------------------------------
// (13 dependent ~20 us launches between the GEMMs kept them from overlapping at their tails)
struct ReduceJob {
    const float* part_w; const float* part_b;
    float* dW; float* db;
    int G, BN, BK, n_out, k_out, ldo, col0;
    int block0;                 // first block of this job in the merged grid
    int overwrite = 0;          // the target is scratch of this call: written whatever ReduceJobs::accumulate says
};
constexpr int kMaxJobs = 16;
struct ReduceJobs { ReduceJob j[kMaxJobs]; int n; int accumulate; };

__global__ __launch_bounds__(256) void wgrad_reduce_multi_kernel(ReduceJobs jobs) {
    int q = 0;
#pragma unroll 1
    for (int i = 1; i < jobs.n; ++i)
        if ((int)blockIdx.x >= jobs.j[i].block0) q = i;
    const ReduceJob& J = jobs.j[q];
    const long idx = (long)(blockIdx.x - J.block0) * blockDim.x + threadIdx.x;
    const long nw = (long)J.n_out * J.k_out;
    if (idx < nw) {
        const int n = (int)(idx / J.k_out), k = (int)(idx % J.k_out);
        float* o = J.dW + (long)n * J.ldo + J.col0 + k;
        const float v = sum_partials(J.part_w + (long)n * J.BK + k, (long)J.BN * J.BK, J.G);
        *o = (jobs.accumulate && !J.overwrite) ? *o + v : v;
        return;
    }
    const long j = idx - nw;
    if (J.db && j < J.n_out) {
        const float v = sum_partials(J.part_b + j, J.BN, J.G);
        J.db[j] = (jobs.accumulate && !J.overwrite) ? J.db[j] + v : v;
    }
}

// ---- the lean group's finishing kernel ---------------------------------------------------------------
// feature_linear has no activation and feeds the views layer linearly (feature = W_f act7 + b_f, d feature = W_vf^T dZv
// with W_vf = views_linears.0.weight[:, :256]), so with the sample sums M = sum_p dZv_p act7_p^T [128][256] and
// s = sum_p dZv_p [128] -- what the views layer's narrow GEMM leaves when its X is act7 --
//   d views_linears.0.weight[:, :256] = M W_f^T + s b_f^T     (128 x 256, K = 256)
//   d feature_linear.weight           = W_vf^T M              (256 x 256, K = 128)
//   d feature_linear.bias             = W_vf^T s,             d views_linears.0.bias = s
// 33 MFLOP on 0.6 MB of operands instead of a 256 x 256 GEMM over all samples and 4 KB of workspace traffic per sample.
// One thread per output element, fp64 accumulation in a fixed order (k ascending): deterministic.  A workgroup owns a
// 16 x 16 tile of one product and stages 16 x 16 operand tiles through LDS so that both operands are read along
// their contiguous axis; the last workgroup forms the two bias vectors.
constexpr int kFinTile = 16;
constexpr int kFinBlocksWF = (256 / kFinTile) * (256 / kFinTile), kFinBlocksWV = (128 / kFinTile) * (256 / kFinTile);
constexpr int kFinLdsBytes = 2 * kFinTile * (kFinTile + 1) * (int)sizeof(float);

template <int PD>
__global__ __launch_bounds__(kFinTile * kFinTile) void wgrad_lean_finish_kernel(const float* __restrict__ M, const float* __restrict__ s,
                                                                                const float* __restrict__ params, float* __restrict__ g,
                                                                                int accumulate) {
    using V = scn::mlp::Var<PD>;
    constexpr int T = kFinTile, LDV = 283;                 // leading dimension of views_linears.0.weight
    const float* W_f = params + V::kWF;
    const float* b_f = params + V::kBF;
    const float* W_vf = params + V::kWV;
    const int tx = threadIdx.x % T, ty = threadIdx.x / T;
    float* As = dynamic_lds<float>();                      // [T][T + 1]: As[r][k]
    float* Bs = As + T * (T + 1);                          // [T][T + 1]: Bs[k][c]
    auto put = [&](float* o, double v) { *o = accumulate ? *o + (float)v : (float)v; };
    int b = blockIdx.x;
    if (b < kFinBlocksWF) {
        // d W_f[i][j] = sum_n W_vf[n][i] M[n][j]: both operands contiguous along the output axes
        const int i0 = (b / (256 / T)) * T, j0 = (b % (256 / T)) * T;
        double acc = 0.0;
        for (int n0 = 0; n0 < 128; n0 += T) {
            As[tx * (T + 1) + ty] = W_vf[(long)(n0 + ty) * LDV + i0 + tx];          // As[i][n]
            Bs[ty * (T + 1) + tx] = M[(n0 + ty) * 256 + j0 + tx];                   // Bs[n][j]
            block_sync();
#pragma unroll
            for (int k = 0; k < T; ++k) acc += (double)As[ty * (T + 1) + k] * (double)Bs[k * (T + 1) + tx];
            block_sync();
        }
        put(g + V::kWF + (i0 + ty) * 256 + j0 + tx, acc);
        return;
    }
    b -= kFinBlocksWF;
    if (b < kFinBlocksWV) {
        // d W_v[n][k] = sum_j M[n][j] W_f[k][j] + s[n] b_f[k]: both operands contiguous along the contraction
        const int n0 = (b / (256 / T)) * T, k0 = (b % (256 / T)) * T;
        double acc = 0.0;
        for (int j0 = 0; j0 < 256; j0 += T) {
            As[ty * (T + 1) + tx] = M[(n0 + ty) * 256 + j0 + tx];                   // As[n][j]
            Bs[tx * (T + 1) + ty] = W_f[(k0 + ty) * 256 + j0 + tx];                 // Bs[j][k]
            block_sync();
#pragma unroll
            for (int k = 0; k < T; ++k) acc += (double)As[ty * (T + 1) + k] * (double)Bs[k * (T + 1) + tx];
            block_sync();
        }
        acc += (double)s[n0 + ty] * (double)b_f[k0 + tx];
        put(g + V::kWV + (long)(n0 + ty) * LDV + k0 + tx, acc);
        return;
    }
    // d b_f[i] = sum_n W_vf[n][i] s[n];  d views bias = s
    const int i = threadIdx.x;
    double acc = 0.0;
    for (int n = 0; n < 128; ++n) acc += (double)W_vf[(long)n * LDV + i] * (double)s[n];
    put(g + V::kBF + i, acc);
    if (i < 128) g[V::kBV + i] = accumulate ? g[V::kBV + i] + s[i] : s[i];
}

template <int PD>
int launch_wgrad_lean_finish(const float* M, const float* s, const float* params, float* g, int accumulate, hipStream_t st) {
    static_assert(kFinTile * kFinTile == 256, "the bias workgroup has one thread per feature");
    hipLaunchKernelGGL((wgrad_lean_finish_kernel<PD>), dim3(kFinBlocksWF + kFinBlocksWV + 1), dim3(kFinTile * kFinTile),
                       kFinLdsBytes, st, M, s, params, g, accumulate);
    return scn_launch_status();
}

// ---- host side: one launcher per kernel family ---------------------------------------------------------
template <int WN, int WK, bool FAST>
int launch_wgrad_impl(const WgradArgs& a, int G, hipStream_t stream) {
    constexpr int BN = 2 * WN * 32, BK = 2 * WK * 32;
    const size_t lds = (size_t)2 * kMS * (BN + 4 + BK + 4) * sizeof(float);
    if (lds > 64 * 1024) SCN_LDS_OPT_IN((wgrad_kernel<WN, WK, FAST>), lds);
    hipLaunchKernelGGL((wgrad_kernel<WN, WK, FAST>), dim3(G), dim3(kThreads), lds, stream, a);
    return scn_launch_status();
}

template <int WN, int WK>
int launch_wgrad(const WgradArgs& a, int G, hipStream_t stream) {
    constexpr int BN = 2 * WN * 32, BK = 2 * WK * 32;
    if (a.a_tiled && a.b_tiled && a.n_load == BN && a.k_load == BK) return launch_wgrad_impl<WN, WK, true>(a, G, stream);
    return launch_wgrad_impl<WN, WK, false>(a, G, stream);
}

// How the 256 x 256 GEMMs (and the narrow ones with a tile-native dZ) multiply: 1 (default) = on three fp16 products per
// product with one power-of-two scale per operand and workgroup chunk, wherever the resident kernels left the chunk maxima
// (wgrad256_half.h, wgrad_half_narrow.h; error vs fp64 equal to the exact-fp32 MFMA kernel's); 0 = v_mfma_f32_32x32x2_f32
// (wgrad256.h, wgrad_tiles.h: the numerical yardstick, and what runs when no maxima were left).  Process-wide;
// SCNERF_WGRAD_ARITHMETIC=fp32 | half presets it, scnerf_wgrad_arithmetic() changes it.
int& wgrad_arithmetic() {
    static int mode = [] {
        const char* e = getenv("SCNERF_WGRAD_ARITHMETIC");
        return (e && (e[0] == 'f' || e[0] == '0')) ? 0 : 1;
    }();
    return mode;
}

// the 256 x 256 tile-native GEMMs of a pass in one launch on the fp32 MFMA, grid (chunks, jobs)
int launch_wgrad256(const wg256::Args& a, int G, hipStream_t stream) {
    constexpr int F = wg256::kSpread;
    SCN_LDS_OPT_IN((wg256::wgrad256_kernel<F>), wg256::kLdsBytes);
    hipLaunchKernelGGL((wg256::wgrad256_kernel<F>), dim3(G, a.n_jobs), dim3(wg256::kThreads), wg256::kLdsBytes, stream, a);
    return scn_launch_status();
}

// the same GEMMs on three fp16 products (wgrad256_half.h): needs the chunk maxima of both operands, [job][chunk]
// xoff (or nullptr): the samples are the live ones of a larger pass -- every job's X is gathered through the table
int launch_wgrad256_half(const wg256::Args& a, int G, const float* amax_a, const float* amax_b, hipStream_t stream,
                         const unsigned* xoff = nullptr) {
    wg256h::Args h;
    for (int j = 0; j < a.n_jobs; ++j) h.job[j] = a.job[j];
    h.n_jobs = a.n_jobs;
    h.Ppad = a.Ppad;
    h.chunk = a.chunk;
    h.amax_a = amax_a;
    h.amax_b = amax_b;
    h.xoff = xoff;
    if (xoff) {
        SCN_LDS_OPT_IN((wg256h::wgrad256_half_kernel<wg256h::kGatherX>), wg256h::kLdsBytes);
        hipLaunchKernelGGL((wg256h::wgrad256_half_kernel<wg256h::kGatherX>), dim3(G, a.n_jobs), dim3(wg256h::kThreads),
                           wg256h::kLdsBytes, stream, h);
        return scn_launch_status();
    }
    SCN_LDS_OPT_IN((wg256h::wgrad256_half_kernel<0>), wg256h::kLdsBytes);
    hipLaunchKernelGGL((wg256h::wgrad256_half_kernel<0>), dim3(G, a.n_jobs), dim3(wg256h::kThreads), wg256h::kLdsBytes,
                       stream, h);
    return scn_launch_status();
}

// narrower shapes with a tile-native dZ (wgrad_tiles.h)
template <int NA, int NB, bool B_ROWMAJOR>
int launch_wgrad_tiles(const wgt::Args& a, int G, hipStream_t stream) {
    constexpr unsigned lds = wgt::lds_bytes<NA, NB, B_ROWMAJOR>();
    if (lds > 64 * 1024) SCN_LDS_OPT_IN((wgt::wgrad_tiles_kernel<NA, NB, B_ROWMAJOR>), lds);
    hipLaunchKernelGGL((wgt::wgrad_tiles_kernel<NA, NB, B_ROWMAJOR>), dim3(G), dim3(wgt::kThreads), lds, stream, a);
    return scn_launch_status();
}

// the same shapes on three fp16 products (wgrad_half_narrow.h); jobs = 2: the pair of GEMMs the arguments name, WB2: the
// second X operand they name
template <int NA, int NB, bool B_ROWMAJOR, int WB2 = 0>
int launch_wgrad_half_narrow(const wgnh::Args& a, int G, hipStream_t stream, int jobs = 1) {
    SCN_LDS_OPT_IN((wgnh::wgrad_half_narrow_kernel<NA, NB, B_ROWMAJOR, WB2>), wgnh::kLdsBytes);
    hipLaunchKernelGGL((wgnh::wgrad_half_narrow_kernel<NA, NB, B_ROWMAJOR, WB2>), dim3(G, jobs), dim3(wgnh::kThreads), wgnh::kLdsBytes, stream, a);
    return scn_launch_status();
}

// the same launch over the live samples of a larger pass: X (and the second X operand) gathered through a.live_idx
template <int NA, int NB, bool B_ROWMAJOR, int WB2 = 0>
int launch_wgrad_half_narrow_live(const wgnh::Args& a, int G, hipStream_t stream, int jobs = 1) {
    SCN_LDS_OPT_IN((wgnh::wgrad_half_narrow_kernel<NA, NB, B_ROWMAJOR, WB2, true>), wgnh::kLdsBytes);
    hipLaunchKernelGGL((wgnh::wgrad_half_narrow_kernel<NA, NB, B_ROWMAJOR, WB2, true>), dim3(G, jobs), dim3(wgnh::kThreads), wgnh::kLdsBytes, stream, a);
    return scn_launch_status();
}

// ---- host side: what a GEMM reads, where its sums go, how the samples are cut, where its partials lie ------
#define SCN_TRY(expr) do { const int rc__ = (expr); SCN_RETURN_IF(rc__ != 0, rc__); } while (0)

struct Operand { const float* p; int ld, load, tiled; };                // tile-native section of width ld, or row-major [P][ld]; `load` columns staged
struct Target { float* dW; int ldo, col0, n_out, k_out; float* db; };   // dW[n * ldo + col0 + k], n < n_out, k < k_out; db [n_out] or nullptr

// THE chunk rule: samples per workgroup when `chunks` workgroups share Ppad samples -- whole LDS stages, never zero.
// The resident kernels index their chunk maxima by the same quantity (scnerf_wgrad_chunk_samples).
long chunk_samples(long Ppad, int chunks) {
    const long chunk = (Ppad + chunks - 1) / chunks;
    return chunk == 0 ? kMS : (chunk + kMS - 1) / kMS * kMS;
}

struct Samples { long P, Ppad; int G; long chunk; };       // valid / padded samples, workgroups, samples per workgroup
Samples cut(long long n_samples, int n_chunks) {
    const long Ppad = scn::mlp::padded_samples((long)n_samples);
    return Samples{(long)n_samples, Ppad, n_chunks, chunk_samples(Ppad, n_chunks)};
}

// the partial sums of one GEMM: w [G][BN][BK], then (bias) b [G][BN]
struct Tile { int G, BN, BK; bool bias; };
struct Slab { float* w; float* b; };
long long slab_floats(const Tile& t) { return (long long)t.G * ((long long)t.BN * t.BK + (t.bias ? t.BN : 0)); }
Slab without_bias(Slab s) { s.b = nullptr; return s; }

// hands out a workspace front to back and refuses to cross `limit`
struct Partials {
    float* next;
    float* limit;
    float* take(long long floats) {
        if (floats > limit - next) return nullptr;
        float* p = next;
        next += floats;
        return p;
    }
    int slab(const Tile& t, Slab* s) {
        s->w = take(slab_floats(t));
        SCN_RETURN_IF(!s->w, SCN_EINVAL);
        s->b = t.bias ? s->w + (long long)t.G * t.BN * t.BK : nullptr;
        return 0;
    }
};

// the one place a ReduceJob is filled
ReduceJob reduce_job(const Slab& s, const Tile& t, const Target& o, int overwrite = 0, int block0 = 0) {
    ReduceJob j;
    j.part_w = s.w; j.part_b = s.b; j.dW = o.dW; j.db = o.db;
    j.G = t.G; j.BN = t.BN; j.BK = t.BK; j.n_out = o.n_out; j.k_out = o.k_out; j.ldo = o.ldo; j.col0 = o.col0;
    j.block0 = block0;
    j.overwrite = overwrite;
    return j;
}
unsigned reduce_blocks(const ReduceJob& j) { return scn_ceil_div((long)j.n_out * j.k_out + (j.db ? j.n_out : 0), 256); }

int launch_reduce(const ReduceJob& j, hipStream_t st) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(reduce_blocks(j)), dim3(256), 0, st, j.part_w, j.part_b, j.G, j.BN, j.BK,
                       j.n_out, j.k_out, j.dW, j.ldo, j.col0, j.db);
    return scn_launch_status();
}

// the reductions of a pass, finished by one launch: push() refuses a job beyond kMaxJobs and places it in the merged grid
struct ReduceQueue {
    ReduceJobs jobs;
    int blocks = 0;
    explicit ReduceQueue(int accumulate) { jobs.n = 0; jobs.accumulate = accumulate; }
    int push(const Slab& s, const Tile& t, const Target& o, int overwrite = 0) {
        SCN_RETURN_IF(jobs.n >= kMaxJobs, SCN_EINVAL);
        jobs.j[jobs.n] = reduce_job(s, t, o, overwrite, blocks);
        blocks += (int)reduce_blocks(jobs.j[jobs.n++]);
        return 0;
    }
};

// where a narrow GEMM finds its operands' maxima (nullptr rows: stay on the fp32 MFMA)
struct NarrowScales {
    wgnh::Bound a, b;
    int n_coarse;
    long coarse_chunk;
};

wgnh::Args narrow_args(const float* dz, const float* x, const Slab& out, const Samples& c, const NarrowScales& ns) {
    const wgnh::Bound none{nullptr, nullptr, nullptr};
    return wgnh::Args{dz, x, out.w, out.b, c.P, c.Ppad, c.chunk, ns.a, ns.b, ns.n_coarse, ns.coarse_chunk,
                      nullptr, nullptr, none, nullptr, nullptr, nullptr, none, nullptr};
}
wgt::Args tiles_args(const float* dz, const float* x, const Slab& out, const Samples& c) {
    return wgt::Args{dz, x, out.w, out.b, c.P, c.Ppad, c.chunk};
}
wg256::Args one_job256(const float* dz, const float* x, const Slab& out, const Samples& c) {
    wg256::Args a;
    a.n_jobs = 1; a.Ppad = c.Ppad; a.chunk = c.chunk;
    a.job[0] = wg256::Job{dz, x, out.w, out.b};
    return a;
}

struct Shape { int BN, BK; };

bool pick_shape(int n_load, int k_load, Shape* s) {
    // (BN, BK) of the six instantiations of wgrad_kernel
    if (n_load > 256 || k_load > 256) return false;
    if (n_load > 128) { s->BN = 256; s->BK = k_load > 128 ? 256 : (k_load > 64 ? 128 : 64); return true; }
    if (n_load > 64) { s->BN = 128; s->BK = k_load > 64 ? 256 : 64; return true; }
    s->BN = 64; s->BK = 128;
    return k_load <= 128;
}

// ---- one GEMM and its reduction, the kernel picked at run time from the operands: the single-GEMM exports, through
// which the tests reach the 256 x 256, tiles, narrow and generic kernels one at a time -------------------------------
int single_gemm(const Operand& dz, const Operand& x, const Target& o, const Samples& c, float* workspace,
                const NarrowScales* narrow, hipStream_t st) {
    SCN_RETURN_IF(!dz.p || !x.p || !workspace || !o.dW || c.P < 0 || c.G < 1, SCN_EINVAL);
    SCN_RETURN_IF(dz.ld % 4 || x.ld % 4 || dz.load % 4 || x.load % 4 || o.n_out > dz.load || o.k_out > x.load, SCN_EINVAL);
    SCN_RETURN_IF(((uintptr_t)dz.p | (uintptr_t)x.p | (uintptr_t)workspace) & 15, SCN_EINVAL);
    Shape s;
    SCN_RETURN_IF(!pick_shape(dz.load, x.load, &s), SCN_ENOSUP);
    // a tile-native operand must fill the block tile exactly (its HBM block is the LDS image)
    SCN_RETURN_IF((dz.tiled && (dz.ld != s.BN || dz.load != dz.ld)) || (x.tiled && (x.ld != s.BK || x.load != x.ld)), SCN_EINVAL);
    const Tile tile{c.G, s.BN, s.BK, true};
    Partials parts{workspace, workspace + slab_floats(tile)};       // (scnerf_wgrad_workspace_floats)
    Slab slab;
    SCN_TRY(parts.slab(tile, &slab));
    const Slab out = o.db ? slab : without_bias(slab);
    const int n = dz.load, k = x.load;
    const bool narrow_shape = dz.tiled && n == dz.ld && k == x.ld &&
                              ((n == 256 && !x.tiled && (k == 64 || k == 128)) || (n == 128 && x.tiled && k == 256));
    int rc;
    if (n == 256 && k == 256 && dz.tiled && x.tiled) {
        rc = launch_wgrad256(one_job256(dz.p, x.p, out, c), c.G, st);
    } else if (narrow_shape && narrow && narrow->a.amax && narrow->b.amax) {
        const wgnh::Args t = narrow_args(dz.p, x.p, out, c, *narrow);
        // (templates are instantiated in the order of first use: this order keeps the code object's layout)
        if (k == 64) rc = launch_wgrad_half_narrow<256, 64, true>(t, c.G, st);
        else if (k == 128) rc = launch_wgrad_half_narrow<256, 128, true>(t, c.G, st);
        else rc = launch_wgrad_half_narrow<128, 256, false>(t, c.G, st);
    } else if (narrow_shape) {
        const wgt::Args t = tiles_args(dz.p, x.p, out, c);
        if (n == 128) rc = launch_wgrad_tiles<128, 256, false>(t, c.G, st);
        else if (k == 64) rc = launch_wgrad_tiles<256, 64, true>(t, c.G, st);
        else rc = launch_wgrad_tiles<256, 128, true>(t, c.G, st);
    } else {
        const WgradArgs a{dz.p, dz.ld, dz.load, dz.tiled, x.p, x.ld, x.load, x.tiled, c.P, c.Ppad, c.chunk, slab.w, slab.b};
        if (s.BN == 256 && s.BK == 256) rc = launch_wgrad<4, 4>(a, c.G, st);
        else if (s.BN == 256 && s.BK == 128) rc = launch_wgrad<4, 2>(a, c.G, st);
        else if (s.BN == 256 && s.BK == 64) rc = launch_wgrad<4, 1>(a, c.G, st);
        else if (s.BN == 128 && s.BK == 256) rc = launch_wgrad<2, 4>(a, c.G, st);
        else if (s.BN == 128 && s.BK == 64) rc = launch_wgrad<2, 1>(a, c.G, st);
        else rc = launch_wgrad<1, 2>(a, c.G, st);
    }
    SCN_RETURN_IF(rc != 0, rc);
    return launch_reduce(reduce_job(slab, tile, o), st);
}

}  // namespace

extern "C" long long scnerf_wgrad_workspace_floats(int n_load, int k_load, int n_chunks) {
    Shape s;
    if (!pick_shape(n_load, k_load, &s) || n_chunks < 1) return -1;
    return slab_floats(Tile{n_chunks, s.BN, s.BK, true});
}

extern "C" long long scnerf_wgrad_chunk_samples(long long n_samples, int n_chunks) {
    if (n_samples < 0 || n_chunks < 1) return -1;
    return chunk_samples(scn::mlp::padded_samples(n_samples), n_chunks);
}

extern "C" int scnerf_wgrad(const float* dz, int lda, int n_load, int n_out, int dz_tiled, const float* x,
                            int ldb, int k_load, int k_out, int x_tiled, long long n_samples, int n_chunks,
                            float* workspace, float* dW, int ldo, int col0, float* db, void* stream) {
    SCN_RETURN_IF(n_samples < 0 || n_chunks < 1, SCN_EINVAL);
    return single_gemm(Operand{dz, lda, n_load, dz_tiled}, Operand{x, ldb, k_load, x_tiled},
                       Target{dW, ldo, col0, n_out, k_out, db}, cut(n_samples, n_chunks), workspace, nullptr,
                       (hipStream_t)stream);
}

// one narrow GEMM (256 x 64 / 256 x 128 with a row-major X, 128 x 256 with a tile-native X) on three fp16 products with
// the maxima given per coarse chunk of coarse_chunk samples (tests: accuracy against fp64); workspace as scnerf_wgrad
extern "C" int scnerf_wgrad_half_narrow(const float* dz_tiled, int n_load, const float* x, int k_load, int k_out,
                                        int x_tiled, long long n_samples, int n_chunks, float* workspace, float* dW,
                                        float* db, const float* amax_dz, const float* amax_x, int n_coarse,
                                        long long coarse_chunk, void* stream) {
    SCN_RETURN_IF(!amax_dz || !amax_x || n_coarse < 1 || coarse_chunk < 32, SCN_EINVAL);
    SCN_RETURN_IF(!((n_load == 256 && !x_tiled && (k_load == 64 || k_load == 128)) || (n_load == 128 && x_tiled && k_load == 256)), SCN_ENOSUP);
    SCN_RETURN_IF(n_samples < 0 || n_chunks < 1, SCN_EINVAL);
    const NarrowScales ns{wgnh::Bound{amax_dz, nullptr, nullptr}, wgnh::Bound{amax_x, nullptr, nullptr}, n_coarse, (long)coarse_chunk};
    return single_gemm(Operand{dz_tiled, n_load, n_load, 1}, Operand{x, k_load, k_load, x_tiled},
                       Target{dW, k_out, 0, n_load, k_out, db}, cut(n_samples, n_chunks), workspace, &ns, (hipStream_t)stream);
}

// one 256 x 256 GEMM on three fp16 products with the chunk maxima given (tests: accuracy against fp64)
extern "C" int scnerf_wgrad256_half(const float* dz_tiled, const float* x_tiled, long long n_samples, int n_chunks,
                                    float* workspace, float* dW, float* db, const float* amax_dz, const float* amax_x,
                                    void* stream) {
    SCN_RETURN_IF(!dz_tiled || !x_tiled || !workspace || !dW || !amax_dz || !amax_x || n_samples < 1 || n_chunks < 1, SCN_EINVAL);
    hipStream_t st = (hipStream_t)stream;
    const Samples c = cut(n_samples, n_chunks);
    const Tile tile{n_chunks, 256, 256, true};
    Partials parts{workspace, workspace + slab_floats(tile)};
    Slab slab;
    SCN_TRY(parts.slab(tile, &slab));
    if (!db) slab = without_bias(slab);
    SCN_TRY(launch_wgrad256_half(one_job256(dz_tiled, x_tiled, slab, c), n_chunks, amax_dz, amax_x, st));
    return launch_reduce(reduce_job(slab, tile, Target{dW, 256, 0, 256, 256, db}), st);
}

extern "C" int scnerf_vecmat(const float* x_tiled256, const float* vec, int vec_stride, long long n_samples,
                             int n_chunks, float* workspace, float* dv, float* dvsum, void* stream) {
    SCN_RETURN_IF(!x_tiled256 || !vec || !workspace || !dv || n_samples < 0 || n_chunks < 1 || vec_stride < 1, SCN_EINVAL);
    const long n_tiles = scn::mlp::padded_samples((long)n_samples) / 32;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vecmat_kernel, dim3(n_chunks), dim3(kThreads), 0, st, x_tiled256, vec, vec_stride,
                       (long)n_samples, n_tiles, workspace);
    hipLaunchKernelGGL(vecmat_reduce_kernel, dim3(2), dim3(256), 0, st, workspace, n_chunks, dv, dvsum, 0);
    return scn_launch_status();
}

// ---- all weight gradients of one network (D=8, W=256, skip 4, view-dependent head; 3-D or 4-D point) ----
extern "C" int scnerf_nerf_param_count(int pt_dims) {
    return pt_dims == 4 ? scn::mlp::Var<4>::kNParams : scn::mlp::Var<3>::kNParams;
}

namespace {
// the GEMM slabs behind the vecmat partials stay 16-byte aligned (the persistent kernel stores them as float4)
long long vecmat_ws_floats(long long n_chunks) { return (257 * n_chunks + 3) / 4 * 4; }

// The 256 x 256 GEMMs of a pass are ONE launch of (chunks, 8) workgroups, one per CU at a time: with an eighth of
// the chunks the narrow GEMMs use, 256 chunks become 32 x 8 = 256 workgroups -- one wave over the chip, every workgroup
// eight times as many samples -- and the partial slabs (256 KB each) shrink from 0.5 GB to 67 MB written and re-read.
int big_chunks(int n_chunks) { return (n_chunks >= 8 && n_chunks % 8 == 0) ? n_chunks / 8 : n_chunks; }

// What scnerf_nerf_wgrad_workspace_floats promises for the partial slabs of a pass (the Python side caches buffers by
// it): the vecmat partials and 9 + 2 + 1 + 1 + 1 slabs at n_chunks.  A pass needs less (its 256 x 256 slabs are cut
// into big_chunks); its Partials take this as their limit, and the lean group's M [128][256] and s [128] lie behind it.
long long partial_floats(long long G) {
    auto blk = [&](long long bn, long long bk) { return G * (bn * bk + bn); };
    return vecmat_ws_floats(G) + 9 * blk(256, 256) + 2 * blk(256, 128) + blk(128, 256) + blk(128, 64) + blk(64, 128);
}
long long lean_scratch_offset(int n_chunks) { return partial_floats(n_chunks); }
constexpr long long kLeanScratchFloats = 128 * 256 + 128;

// what every pass is given: the workspaces of its forward / backward, d raw [P][4], the samples and their chunks, the
// workspace of this group (scnerf_nerf_wgrad_workspace_floats(n_chunks)) and the flat gradient
struct PassBuffers {
    const float* save; const float* grads; const float* d_raw;
    long long P; int n_chunks;
    float* workspace; float* g; int accumulate;
    hipStream_t st;
};

// amax_x / amax_z (or nullptr): [8][big_chunks] chunk maxima of the X / dZ operands of the 256 x 256 GEMMs in the order of
// the big launch (layers 1 .. 7, feature_linear), left by the resident kernels: with them that launch runs on three fp16
// products (wgrad256_half.h) unless the arithmetic is switched to fp32.  With `scales` as well (rows 8 .. 11 of amax_z:
// dZ of the views layer, dZ of layer 0, max(1, |point|) >= the encoded point, the encoded direction's bound --
// mlp_bwd_h3_kernel.h; the feature is bounded through its layer) so do the narrow GEMMs.
// ev_before / ev_after (or nullptr): events recorded around the big launch (bench.py's per-kernel timing) -- arguments
// of THIS call, so that no exit path can leave them armed for a later one.
// lean_params (the flat parameter buffer of the network that ran the pass): the LEAN group for workspaces whose
// feature / d feature sections were not stored -- no feature_linear job (seven in the big launch, same chunking: the
// other gradients stay bit-identical), the views layer's narrow GEMM on act7 into scratch, wgrad_lean_finish_kernel.
// live (idx != nullptr): the pass runs on the LIVE samples of a larger one (live_compact.hip).  `grads`, P, the chunks
// and both maxima tables belong to the compact batch; `save` and `d_raw` are the dense ones of the P_src samples of the
// forward.  Every GEMM gathers its X through idx / xoff; vecmat and rows4, which read only X and d_raw, stay dense over
// P_src in n_chunks_src workgroups (alpha_linear and rgb_linear keep the dense group's bits); the workspace is the one
// of n_chunks_src >= n_chunks.
struct LiveSamples { const int* idx; const unsigned* xoff; long long P_src; int n_chunks_src; };
constexpr long long kLiveMaxSamples = (1LL << 22) - 128;       // 1 KB per sample and 256-wide section: offsets below 2^32
struct PassOptions {
    const float* amax_x; const float* amax_z; const float* scales;
    hipEvent_t ev_before, ev_after;
    const float* lean_params;
    LiveSamples live;
};

// A pass lays out its slabs and reduction jobs first, in the order of the flat gradient, then launches: layer 0 with the skip
// columns, vecmat, the views layer, rows4, the big launch (trunk layers 1 .. 7 and, not lean, feature_linear), the one
// reduction and, lean, the finishing kernel.
template <int PD>
int nerf_wgrad(const PassBuffers& io, const PassOptions& o) {
    using namespace scn::mlp;
    using V = Var<PD>;
    constexpr int EW = V::kEW, IN = V::kInCh, SK = V::kSkipLd;
    const bool lean = o.lean_params != nullptr;
    const bool half_big = o.amax_x && o.amax_z && wgrad_arithmetic() == 1;
    const bool half_narrow = half_big && o.scales;
    SCN_RETURN_IF(lean && !half_narrow, SCN_EINVAL);     // (a lean workspace has no feature sections for the full group)
    const bool live = o.live.idx != nullptr;
    SCN_RETURN_IF(live && (!half_narrow || !o.live.xoff || o.live.P_src < io.P || o.live.n_chunks_src < io.n_chunks), SCN_EINVAL);
    const int nc = io.n_chunks, nb = big_chunks(nc);
    const int nc_src = live ? o.live.n_chunks_src : nc;
    const Samples fine = cut(io.P, nc), coarse = cut(io.P, nb);
    const Samples src = live ? cut(o.live.P_src, nc_src) : fine;       // what `save` and `d_raw` cover
    auto sv = [&](int sec) { return io.save + (long long)sec * src.Ppad; };
    auto gr = [&](int sec) { return io.grads + (long long)sec * fine.Ppad; };
    auto act = [&](int l) { return sv(kSaveAct + 256 * l); };
    auto dz = [&](int l) { return gr(kGradDz + 256 * l); };
    auto zrow = [&](int r) { return wgnh::Bound{o.amax_z + (long)r * nb, nullptr, nullptr}; };
    float* const g = io.g;
    float* const scratch = io.workspace + lean_scratch_offset(nc_src);
    hipStream_t st = io.st;

    Partials parts{io.workspace, scratch};
    ReduceQueue red(io.accumulate);
    auto plan = [&](const Tile& t, const Target& out, Slab* s, int overwrite = 0) -> int {
        SCN_TRY(parts.slab(t, s));
        return red.push(*s, t, out, overwrite);
    };
    wg256::Args big;                 // the 256 x 256 GEMMs go out as one launch
    big.n_jobs = 0; big.Ppad = coarse.Ppad; big.chunk = coarse.chunk;
    auto plan_big = [&](const float* dzl, const float* x, const Target& out) -> int {
        SCN_RETURN_IF(big.n_jobs >= wg256::kMaxJobs, SCN_EINVAL);
        Slab s;
        SCN_TRY(plan(Tile{nb, 256, 256, true}, out, &s));
        big.job[big.n_jobs++] = wg256::Job{dzl, x, s.w, s.b};
        return 0;
    };
    auto trunk = [&](int l, int col0) { return Target{g + V::trunk_w(l), l == 5 ? SK : 256, col0, 256, 256, g + V::trunk_b(l)}; };

    float* const vm = parts.take(vecmat_ws_floats(nc_src));       // [G][257]: the vecmat partials
    SCN_RETURN_IF(!vm, SCN_EINVAL);
    Slab s_l0, s_skip;
    SCN_TRY(plan(Tile{nc, 256, EW, true}, Target{g + V::kW0, IN, 0, 256, IN, g + V::kB0}, &s_l0));
    for (int l = 1; l <= 4; ++l) SCN_TRY(plan_big(dz(l), act(l - 1), trunk(l, 0)));
    SCN_TRY(plan(Tile{nc, 256, EW, true}, Target{g + V::trunk_w(5), SK, 0, 256, IN, nullptr}, &s_skip));
    SCN_TRY(plan_big(dz(5), act(4), trunk(5, IN)));
    for (int l = 6; l <= 7; ++l) SCN_TRY(plan_big(dz(l), act(l - 1), trunk(l, 0)));
    if (!lean) SCN_TRY(plan_big(gr(kGradDfeat), act(7), Target{g + V::kWF, 256, 0, 256, 256, g + V::kBF}));

    // layer 0 and the skip columns of layer 5: X = encoded points (row-major, IN valid of EW columns).  Half arithmetic: ONE
    // narrow launch, grid (G, 2), whose workgroups pair up on a CU and read X once; otherwise two wgrad_tiles launches
    if (half_narrow) {
        wgnh::Args both = narrow_args(dz(0), sv(kSaveEpts), s_l0, fine, NarrowScales{zrow(9), zrow(10), nb, coarse.chunk});
        both.A_y1 = dz(5); both.part_w_y1 = s_skip.w; both.part_b_y1 = nullptr; both.a_y1 = zrow(4);
        both.live_idx = o.live.idx;
        SCN_TRY(live ? (launch_wgrad_half_narrow_live<256, EW, true>(both, nc, st, 2))
                     : (launch_wgrad_half_narrow<256, EW, true>(both, nc, st, 2)));
    } else {
        SCN_TRY((launch_wgrad_tiles<256, EW, true>(tiles_args(dz(0), sv(kSaveEpts), s_l0, fine), nc, st)));
        SCN_TRY((launch_wgrad_tiles<256, EW, true>(tiles_args(dz(5), sv(kSaveEpts), without_bias(s_skip), fine), nc, st)));
    }
    // alpha_linear (one output row) = d sigma^T . act7 with d sigma = d_raw[:, 3]: the 256 sums and the bias sum as two jobs
    hipLaunchKernelGGL(vecmat_kernel, dim3(nc_src), dim3(kThreads), 0, st, act(7), io.d_raw + 3, 4, src.P, src.Ppad / 32, vm);
    SCN_TRY(scn_launch_status());
    SCN_TRY(red.push(Slab{vm, nullptr}, Tile{nc_src, 1, 257, false}, Target{g + V::kWA, 256, 0, 1, 256, nullptr}));
    SCN_TRY(red.push(Slab{vm + 256, nullptr}, Tile{nc_src, 1, 257, false}, Target{g + V::kBA, 1, 0, 1, 1, nullptr}));
    // views layer: X = [feature | encoded direction].  Half arithmetic: one narrow launch with the direction as second X
    // operand (WB2 = 32), dZ is read (and cut) once; otherwise wgrad_tiles<128, 256> and the generic 128 x 64 kernel
    const Target views_dir{g + V::kWV, 283, 256, 128, 27, nullptr};
    Slab s_feat, s_dir;
    if (half_narrow) {
        // (lean: X = act7, bounded by its own maxima -- row 7 of the X table -- instead of the feature behind it, and the
        // sums M and s go to the scratch whatever `accumulate` says)
        const float* bound = o.scales + scn::h3::kLayerFeat * scn::h3::kScaleStride;
        const wgnh::Bound b_feat{o.amax_x + 7L * nb, bound + scn::h3::kBoundA, bound + scn::h3::kBoundB};
        const wgnh::Bound b_act7{o.amax_x + 7L * nb, nullptr, nullptr};
        SCN_TRY(plan(Tile{nc, 128, 256, true}, lean ? Target{scratch, 256, 0, 128, 256, scratch + 128 * 256}
                                                    : Target{g + V::kWV, 283, 0, 128, 256, g + V::kBV}, &s_feat, lean));
        SCN_TRY(plan(Tile{nc, 128, 32, false}, views_dir, &s_dir));
        wgnh::Args t = narrow_args(gr(kGradDzv), lean ? act(7) : sv(kSaveFeat), s_feat, fine,
                                   NarrowScales{zrow(8), lean ? b_act7 : b_feat, nb, coarse.chunk});
        t.B2 = sv(kSaveEviews); t.part_w2 = s_dir.w; t.b2 = zrow(11);
        t.live_idx = o.live.idx;
        SCN_TRY(live ? (launch_wgrad_half_narrow_live<128, 256, false, 32>(t, nc, st))
                     : (launch_wgrad_half_narrow<128, 256, false, 32>(t, nc, st)));
    } else {
        SCN_TRY(plan(Tile{nc, 128, 256, true}, Target{g + V::kWV, 283, 0, 128, 256, g + V::kBV}, &s_feat));
        SCN_TRY(plan(Tile{nc, 128, 64, true}, views_dir, &s_dir));
        SCN_TRY((launch_wgrad_tiles<128, 256, false>(tiles_args(gr(kGradDzv), sv(kSaveFeat), s_feat, fine), nc, st)));
        const WgradArgs a{gr(kGradDzv), 128, 128, 1, sv(kSaveEviews), 32, 32, 0, fine.P, fine.Ppad, fine.chunk, s_dir.w, s_dir.b};
        SCN_TRY((launch_wgrad<2, 1>(a, nc, st)));
    }
    // rgb_linear: dZ = d_raw[:, 0:3] (row-major), X = hidden of the views layer
    // (rows4_kernel: the hidden layer is read once at the HBM rate; the general kernel pads three rows to a 64-row tile)
    Slab s_rgb;
    SCN_TRY(plan(Tile{nc_src, 4, 128, true}, Target{g + V::kWRGB, 128, 0, 3, 128, g + V::kBRGB}, &s_rgb));
    hipLaunchKernelGGL(rows4_kernel, dim3(nc_src), dim3(kThreads), 0, st, sv(kSaveHv), io.d_raw, src.P, src.Ppad / 32, s_rgb.w, s_rgb.b);
    SCN_TRY(scn_launch_status());
    if (o.ev_before) SCN_HIP(hipEventRecord(o.ev_before, st));
    SCN_TRY(half_big ? launch_wgrad256_half(big, nb, o.amax_z, o.amax_x, st, o.live.xoff) : launch_wgrad256(big, nb, st));
    if (o.ev_after) SCN_HIP(hipEventRecord(o.ev_after, st));
    // one launch finishes every GEMM (fixed-order sums: deterministic)
    hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3(red.blocks), dim3(256), 0, st, red.jobs);
    SCN_TRY(scn_launch_status());
    if (!lean) return 0;
    // (both variants: the three parameters sit at Var<PD>'s offsets, the views layer is 283 columns wide in either)
    return launch_wgrad_lean_finish<PD>(scratch, scratch + 128 * 256, o.lean_params, g, io.accumulate, st);
}

// the one body of the three exports below
int nerf_wgrad_entry(int pt_dims, const PassBuffers& io, const PassOptions& o) {
    SCN_RETURN_IF(!io.save || !io.grads || !io.d_raw || !io.workspace || !io.g || io.P < 1 || io.n_chunks < 1, SCN_EINVAL);
    SCN_RETURN_IF(pt_dims != 3 && pt_dims != 4, SCN_EINVAL);
    return pt_dims == 3 ? nerf_wgrad<3>(io, o) : nerf_wgrad<4>(io, o);
}
}  // namespace

extern "C" int scnerf_nerf_wgrad(int pt_dims, const float* save, const float* grads, const float* d_raw,
                                 long long n_samples, int n_chunks, float* workspace, float* flat_grad,
                                 int accumulate, void* stream) {
    return nerf_wgrad_entry(pt_dims, PassBuffers{save, grads, d_raw, n_samples, n_chunks, workspace, flat_grad, accumulate, (hipStream_t)stream},
                            PassOptions{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int scnerf_nerf_wgrad_h3(int pt_dims, const float* save, const float* grads, const float* d_raw,
                                    long long n_samples, int n_chunks, float* workspace, float* flat_grad,
                                    int accumulate, const float* amax_x, const float* amax_z, const float* scales,
                                    void* ev_before, void* ev_after, void* stream) {
    return nerf_wgrad_entry(pt_dims, PassBuffers{save, grads, d_raw, n_samples, n_chunks, workspace, flat_grad, accumulate, (hipStream_t)stream},
                            PassOptions{amax_x, amax_z, scales, (hipEvent_t)ev_before, (hipEvent_t)ev_after, nullptr});
}

// the lean group (include/scnerf_hip.h): either network variant, all three tables, the half arithmetic
extern "C" int scnerf_nerf_wgrad_h3_lean(int pt_dims, const float* save, const float* grads, const float* d_raw,
                                         long long n_samples, int n_chunks, float* workspace, float* flat_grad,
                                         int accumulate, const float* amax_x, const float* amax_z, const float* scales,
                                         const float* flat_params, void* ev_before, void* ev_after, void* stream) {
    SCN_RETURN_IF(!amax_x || !amax_z || !scales || !flat_params || wgrad_arithmetic() != 1, SCN_EINVAL);
    return nerf_wgrad_entry(pt_dims, PassBuffers{save, grads, d_raw, n_samples, n_chunks, workspace, flat_grad, accumulate, (hipStream_t)stream},
                            PassOptions{amax_x, amax_z, scales, (hipEvent_t)ev_before, (hipEvent_t)ev_after, flat_params});
}

// the group over the live samples of a pass (include/scnerf_hip.h): the half arithmetic and all three tables required;
// flat_params NULL: the full group, else the lean one
extern "C" int scnerf_nerf_wgrad_h3_live(int pt_dims, const float* save, long long n_samples_src, int n_chunks_src,
                                         const float* grads_live, const float* d_raw, const int* live_idx,
                                         const unsigned* xoff, long long n_live, int n_chunks_live, float* workspace,
                                         float* flat_grad, int accumulate, const float* amax_x_live, const float* amax_z_live,
                                         const float* scales, const float* flat_params, void* ev_before, void* ev_after,
                                         void* stream) {
    SCN_RETURN_IF(!amax_x_live || !amax_z_live || !scales || !live_idx || !xoff || wgrad_arithmetic() != 1, SCN_EINVAL);
    SCN_RETURN_IF(n_live < 1 || n_live > n_samples_src || n_chunks_live < 1 || n_chunks_live > n_chunks_src, SCN_EINVAL);
    SCN_RETURN_IF(n_samples_src > kLiveMaxSamples, SCN_ENOSUP);      // (the byte offsets of a 256-wide section fit 32 bits)
    return nerf_wgrad_entry(pt_dims, PassBuffers{save, grads_live, d_raw, n_live, n_chunks_live, workspace, flat_grad, accumulate, (hipStream_t)stream},
                            PassOptions{amax_x_live, amax_z_live, scales, (hipEvent_t)ev_before, (hipEvent_t)ev_after, flat_params,
                                        LiveSamples{live_idx, xoff, n_samples_src, n_chunks_src}});
}

extern "C" int scnerf_wgrad_arithmetic(int mode) {
    if (mode == 0 || mode == 1) wgrad_arithmetic() = mode;
    return wgrad_arithmetic();
}

extern "C" int scnerf_wgrad256_chunks(int n_chunks) { return n_chunks < 1 ? -1 : big_chunks(n_chunks); }

extern "C" int scnerf_wgrad_lean_finish_pd(int pt_dims, const float* M, const float* s, const float* flat_params,
                                           float* flat_grad, int accumulate, void* stream) {
    SCN_RETURN_IF(!M || !s || !flat_params || !flat_grad || (pt_dims != 3 && pt_dims != 4), SCN_EINVAL);
    if (pt_dims == 3) return launch_wgrad_lean_finish<3>(M, s, flat_params, flat_grad, accumulate, (hipStream_t)stream);
    return launch_wgrad_lean_finish<4>(M, s, flat_params, flat_grad, accumulate, (hipStream_t)stream);
}

extern "C" int scnerf_wgrad_lean_finish(const float* M, const float* s, const float* flat_params, float* flat_grad,
                                        int accumulate, void* stream) {
    return scnerf_wgrad_lean_finish_pd(3, M, s, flat_params, flat_grad, accumulate, stream);
}

// the partial slabs of a pass (see partial_floats) + the lean group's scratch (M [128][256], s [128])
extern "C" long long scnerf_nerf_wgrad_workspace_floats(int n_chunks) {
    return partial_floats(n_chunks) + kLeanScratchFloats;
}
