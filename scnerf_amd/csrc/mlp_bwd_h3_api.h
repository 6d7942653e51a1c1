// mlp_bwd_h3_api.h -- shared by the translation units of the resident data-gradient chain.
#pragma once
#include <hip/hip_runtime.h>

#include "resident_guard.h"

namespace scn {
namespace h3b {

// Where the weight-gradient GEMMs' chunk maxima of the dZ operands go (wgrad256_half.h): amax [8][n_chunks], job j =
// dZ of trunk layer j + 1 (j = 7: d feature); chunk = samples per weight-gradient workgroup.
// `guard`: the record of the scale guard (resident_guard.h; null pointers: no check).
// `lean`: the d feature section is not stored (the lean weight-gradient group of wgrad.hip does not read it); every
// other output is bit-identical.  (In the padding behind n_chunks: the argument block keeps its layout.)
struct ChunkMaxima { float* amax; int n_chunks; int lean; long chunk; ResidentGuard guard; };

int bwd_h3_pd3(const float* d_raw, const float* pts, const float* viewdirs, int vd_stride, int samples_per_ray,
               const float* wpacked_bwd, const short* stream_bwd, const float* scales, const float* save, float* grads,
               float* d_pts, float* d_views, long long n_samples, ChunkMaxima cm, hipStream_t st);
int bwd_h3_pd4(const float* d_raw, const float* pts, const float* viewdirs, int vd_stride, int samples_per_ray,
               const float* wpacked_bwd, const short* stream_bwd, const float* scales, const float* save, float* grads,
               float* d_pts, float* d_views, long long n_samples, ChunkMaxima cm, hipStream_t st);

}  // namespace h3b
}  // namespace scn
