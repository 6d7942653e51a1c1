// philox.h -- Philox4x32-10 (Salmon et al., SC'11), the counter-based generator of randoms.hip (the draws of a render_rays
// call) and ray_batch.hip (the round function of the batch permutation).  One definition, so that the two files cannot
// drift apart: ten rounds, the multipliers and Weyl key increments of the paper; a pure function of (counter, key).
#pragma once

namespace scn {

struct U4 { unsigned x, y, z, w; };

__host__ __device__ inline unsigned mulhi32(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

__host__ __device__ inline U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = mulhi32(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = mulhi32(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

}  // namespace scn
