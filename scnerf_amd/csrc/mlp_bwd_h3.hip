// mlp_bwd_h3.hip -- the data-gradient chain of the NeRF MLP in the "resident" arithmetic (mlp_h3.h): d raw ->
// rgb^T -> views^T -> feature^T (+ the density head's rank-1 term) -> trunk layers 7^T .. 1^T with the ReLU gates ->
// layer 0^T and the skip columns -> the encoding's gradient -> d pts, d viewdirs, as ONE launch on three fp16
// products per product.  The gradient w.r.t. a layer's output lives in registers as cut fp16 planes and is the B
// operand of the transposed layer; every dZ the weight-gradient GEMMs need is written once (tile-native sections of
// mlp_common.h, as mlp_bwd.hip) and never read back here.
//
// Gradient of: NeRF.forward + Embedder + run_network
//   /root/reference NeRF/run_nerf_helpers.py:105-128, :24-72, NeRF/create_nerf.py:18-32 (what autograd derives).
#include <cstdint>

#include <scn_wave.h>

#include "launch.h"
#include "mlp_bwd_h3_api.h"
#include "mlp_common.h"
#include "scnerf_hip.h"

extern "C" int scnerf_mlp_bwd_h3_lean(int pt_dims, const float* d_raw, const float* pts, const float* viewdirs,
                                      int vd_stride, int samples_per_ray, const float* wpacked_bwd, const short* stream_bwd,
                                      const float* scales, const float* save, float* grads, float* d_pts, float* d_views,
                                      long long n_samples, float* chunk_amax, int n_chunks, long long chunk_samples,
                                      int* guard_flags, int* guard_any, float* guard_report, int lean, void* stream) {
    SCN_RETURN_IF(!d_raw || !pts || !viewdirs || !wpacked_bwd || !stream_bwd || !scales || !save || !grads, SCN_EINVAL);
    SCN_RETURN_IF(!d_pts != !d_views, SCN_EINVAL);             // both NULL: no input gradient
    SCN_RETURN_IF(samples_per_ray < 1 || vd_stride < 3 || n_samples < 0 || (pt_dims != 3 && pt_dims != 4), SCN_EINVAL);
    SCN_RETURN_IF(n_samples >= (1LL << 31), SCN_ENOSUP);       // (the kernel indexes samples with 31 bits)
    SCN_RETURN_IF(chunk_amax && (n_chunks < 1 || chunk_samples < 32 || chunk_samples % 32), SCN_EINVAL);
    SCN_RETURN_IF(!guard_flags != !guard_any || (guard_report && !guard_flags), SCN_EINVAL);
    if (n_samples == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const scn::h3b::ChunkMaxima cm{chunk_amax, n_chunks, lean != 0, (long)chunk_samples, {guard_flags, guard_any, guard_report}};
    return pt_dims == 3 ? scn::h3b::bwd_h3_pd3(d_raw, pts, viewdirs, vd_stride, samples_per_ray, wpacked_bwd, stream_bwd, scales, save, grads, d_pts, d_views, n_samples, cm, st)
                        : scn::h3b::bwd_h3_pd4(d_raw, pts, viewdirs, vd_stride, samples_per_ray, wpacked_bwd, stream_bwd, scales, save, grads, d_pts, d_views, n_samples, cm, st);
}

// The same launch with the ReLU masks in a buffer of their own (nine lane-native sections over padded n_samples, as
// behind the row sections of a workspace): the batch of live samples of live_compact.hip has no workspace.  The kernel
// reads nothing but the masks through `save`, at save + kSavePerSample * Ppad: it is handed the address that puts them
// there.  A guard record here has one flag per 128 samples of THIS batch.
extern "C" int scnerf_mlp_bwd_h3_masks(int pt_dims, const float* d_raw, const float* pts, const float* viewdirs,
                                       int vd_stride, int samples_per_ray, const float* wpacked_bwd, const short* stream_bwd,
                                       const float* scales, const unsigned* masks, float* grads, float* d_pts, float* d_views,
                                       long long n_samples, float* chunk_amax, int n_chunks, long long chunk_samples,
                                       int* guard_flags, int* guard_any, float* guard_report, int lean, void* stream) {
    SCN_RETURN_IF(!masks || n_samples < 0 || (pt_dims != 3 && pt_dims != 4), SCN_EINVAL);
    const long long per_sample = pt_dims == 3 ? scn::mlp::Var<3>::kSavePerSample : scn::mlp::Var<4>::kSavePerSample;
    const uintptr_t base = reinterpret_cast<uintptr_t>(masks) - (uintptr_t)(per_sample * scn::mlp::padded_samples((long)n_samples)) * sizeof(float);
    return scnerf_mlp_bwd_h3_lean(pt_dims, d_raw, pts, viewdirs, vd_stride, samples_per_ray, wpacked_bwd, stream_bwd, scales,
                                  reinterpret_cast<const float*>(base), grads, d_pts, d_views, n_samples, chunk_amax, n_chunks,
                                  chunk_samples, guard_flags, guard_any, guard_report, lean, stream);
}

extern "C" int scnerf_mlp_bwd_h3_guarded(int pt_dims, const float* d_raw, const float* pts, const float* viewdirs,
                                         int vd_stride, int samples_per_ray, const float* wpacked_bwd, const short* stream_bwd,
                                         const float* scales, const float* save, float* grads, float* d_pts, float* d_views,
                                         long long n_samples, float* chunk_amax, int n_chunks, long long chunk_samples,
                                         int* guard_flags, int* guard_any, float* guard_report, void* stream) {
    return scnerf_mlp_bwd_h3_lean(pt_dims, d_raw, pts, viewdirs, vd_stride, samples_per_ray, wpacked_bwd, stream_bwd, scales, save,
                                  grads, d_pts, d_views, n_samples, chunk_amax, n_chunks, chunk_samples, guard_flags, guard_any,
                                  guard_report, 0, stream);
}

extern "C" int scnerf_mlp_bwd_h3(int pt_dims, const float* d_raw, const float* pts, const float* viewdirs, int vd_stride,
                                 int samples_per_ray, const float* wpacked_bwd, const short* stream_bwd, const float* scales,
                                 const float* save, float* grads, float* d_pts, float* d_views, long long n_samples,
                                 float* chunk_amax, int n_chunks, long long chunk_samples, void* stream) {
    return scnerf_mlp_bwd_h3_guarded(pt_dims, d_raw, pts, viewdirs, vd_stride, samples_per_ray, wpacked_bwd, stream_bwd, scales,
                                     save, grads, d_pts, d_views, n_samples, chunk_amax, n_chunks, chunk_samples, nullptr,
                                     nullptr, nullptr, stream);
}
