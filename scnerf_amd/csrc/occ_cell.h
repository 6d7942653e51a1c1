// occ_cell.h -- the occupancy grid's cell test of one sample, shared by occupancy.hip (ops.inference_occupancy) and
// early_stop.hip (ops.inference_early_stop with a grid), so that both ask the SAME instructions whether a sample is live.
//
// The grid: one bit per cell of an R x R x R lattice over the box [lo, hi), R a multiple of 32.  Cell (x, y, z) is bit
// c & 31 of word c >> 5, c = (z R + y) R + x; the words are int32.  A sample with point p is DEAD only when all three
// t_a = (p_a - lo_a) * inv_a -- one fp32 subtraction, one fp32 multiplication, each rounded, never fused -- satisfy
// 0 <= t_a < R and the bit of cell (floor t_x, floor t_y, floor t_z) is 0.  A NaN coordinate and a point outside the box are
// live.  inv_a = R / (hi_a - lo_a) is the caller's (computed once, in fp32, on the host).
#pragma once
#include <hip/hip_runtime.h>

namespace scn {
namespace occ {

// a - b, a * b and a + b, each rounded once (the build runs with -ffp-contract=off; on the device the intrinsics say so again)
__device__ __forceinline__ float sub_rn(float a, float b) {
#if defined(SCNERF_SIMT_EMU_BUILD)
    return a - b;
#else
    return __fsub_rn(a, b);
#endif
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#if defined(SCNERF_SIMT_EMU_BUILD)
    return a * b;
#else
    return __fmul_rn(a, b);
#endif
}
__device__ __forceinline__ float add_rn(float a, float b) {
#if defined(SCNERF_SIMT_EMU_BUILD)
    return a + b;
#else
    return __fadd_rn(a, b);
#endif
}

struct Grid {
    const unsigned* bits;        // [R^3 / 32]
    int R;
    float lo_x, lo_y, lo_z, inv_x, inv_y, inv_z;
};

__device__ __forceinline__ bool sample_live(const Grid& g, const float* __restrict__ pts, long i) {
    const float fr = (float)g.R;
    const float tx = mul_rn(sub_rn(pts[3 * i + 0], g.lo_x), g.inv_x);
    const float ty = mul_rn(sub_rn(pts[3 * i + 1], g.lo_y), g.inv_y);
    const float tz = mul_rn(sub_rn(pts[3 * i + 2], g.lo_z), g.inv_z);
    const bool inside = tx >= 0.f && tx < fr && ty >= 0.f && ty < fr && tz >= 0.f && tz < fr;      // (false with a NaN)
    if (!inside) return true;
    // 0 <= t < R: the conversion truncates towards zero, which is floor here (-0.0 -> cell 0)
    const long c = ((long)(int)tz * g.R + (int)ty) * g.R + (int)tx;
    return ((g.bits[c >> 5] >> (unsigned)(c & 31)) & 1u) != 0u;
}

// The inverted-sphere space of the NeRF++ background network (csrc/npp_occupancy.hip): a sample is (x', y', z', w), a unit
// direction and w = 1 / r in [0, 1]; q = (x' w, y' w, z' w) -- one fp32 multiplication per axis, rounded once -- maps the
// outside of the unit sphere onto the unit ball, and q takes sample_live's test on the same R^3 bit lattice over a box in q.
// A NaN component and a q outside the box are live; w = 0 gives q = +-0, inside when lo < 0 < hi.
__device__ __forceinline__ bool sample_live_inverted(const Grid& g, float px, float py, float pz, float pw) {
    const float fr = (float)g.R;
    const float tx = mul_rn(sub_rn(mul_rn(px, pw), g.lo_x), g.inv_x);
    const float ty = mul_rn(sub_rn(mul_rn(py, pw), g.lo_y), g.inv_y);
    const float tz = mul_rn(sub_rn(mul_rn(pz, pw), g.lo_z), g.inv_z);
    const bool inside = tx >= 0.f && tx < fr && ty >= 0.f && ty < fr && tz >= 0.f && tz < fr;      // (false with a NaN)
    if (!inside) return true;
    const long c = ((long)(int)tz * g.R + (int)ty) * g.R + (int)tx;
    return ((g.bits[c >> 5] >> (unsigned)(c & 31)) & 1u) != 0u;
}

static inline bool bad_resolution(int R) { return R < 32 || R > 1024 || (R & 31) != 0; }

}  // namespace occ
}  // namespace scn
