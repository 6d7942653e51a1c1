// resident_guard.h -- the run-time check of the resident arithmetic's per-sample scales (mlp_h3.h).
//
// A layer output cut at the per-sample power of two S is fp32 grade while the sample's log2(max|z| S) lies in
// [kGuardLo, kGuardHi) (mlp_h3.h:18-26).  S comes from a bound known before the layer runs; the upper end holds by
// construction, the lower end only while the bound is not far looser than the values.  The consuming layer measures
// max|z| anyway (the chunk maxima), so the check costs a compare and a ballot per layer and wave:
//     m = exponent(max|z|) + exponent(S),   the sample trips if m < kGuardLo or m >= kGuardHi   (live samples, max|z| > 0)
// What a guarded launch leaves (a null `flags` turns the check off; `report` may be null):
//   flags   int [ceil(P / 128)]: 1 for every 128-sample block holding a tripped sample (plain stores, idempotent)
//   any     int [1]: 1 when any sample of the launch tripped
//   report  float [kGuardLayers][kGuardSlots]: the largest kGuardBias - m (one atomic max per wave and layer, spread over
//           the slots by wave tile), then float [kGuardLayers][2]: the samples under / over (an atomic only from a wave
//           that tripped).  Zero-filled by the caller; floats so that the existing max / add atomics serve (counts exact
//           to 2^24 per layer).
// Layers: 0 .. 7 trunk, 8 feature, 9 views -- in the data-gradient chain the same indices name dZ of that layer.
#pragma once

namespace scn {

struct ResidentGuard { int* flags; int* any; float* report; };

constexpr int kGuardLo = -3, kGuardHi = 13;
constexpr int kGuardLayers = 10, kGuardSlots = 64;
constexpr int kGuardBias = 256;                    // kGuardBias - m >= 0 for every max|z| and S the kernels form
constexpr int kGuardReportFloats = kGuardLayers * kGuardSlots + kGuardLayers * 2;

}  // namespace scn
