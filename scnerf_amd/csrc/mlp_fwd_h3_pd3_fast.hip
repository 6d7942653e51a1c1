// mlp_fwd_h3_pd3_fast.hip -- one instantiation group of the resident forward kernel (mlp_fwd_h3_kernel.h): the
// forward-only sample-list forward on ONE fp16 product per product, 3-D points.
#include "mlp_fwd_h3_kernel.h"

namespace scn {
namespace h3f {

int fwd_h3_pd3_fast(const float* pts, const float* viewdirs, int vd_stride, int samples_per_ray, const float* wpacked,
                    const short* stream_fwd, const float* scales, float* raw, long long n_samples, hipStream_t st) {
    return launch_fwd_h3<3, false, 1>(pts, viewdirs, vd_stride, samples_per_ray, wpacked, stream_fwd, scales, raw, nullptr, n_samples,
                                      ChunkMaxima{}, st);
}

}  // namespace h3f
}  // namespace scn
