// mlp_fwd_h3_coarse_fast.hip -- one instantiation group of the resident forward kernel (mlp_fwd_h3_kernel.h): the
// forward-only fused coarse stage on ONE fp16 product per product.
#include "mlp_fwd_h3_kernel.h"

namespace scn {
namespace h3f {

int fwd_h3_coarse_fast(const CoarseStage& cs, const float* rays, int ray_stride, const float* wpacked, const short* stream_fwd,
                       const float* scales, float* raw, hipStream_t st) {
    return launch_coarse_h3<false, 1>(cs, rays, ray_stride, wpacked, stream_fwd, scales, raw, nullptr, ChunkMaxima{}, st);
}

}  // namespace h3f
}  // namespace scn
