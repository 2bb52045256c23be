// pt_moments.hpp — the per-pixel sample moments (RT_OPT_MOMENTS): the ONE place two partial states of a pixel are combined.
// A state is (n, S, M2): n samples, their RGB sum S, and the centred second moment of their luminances,
// M2 = sum_j (l(s_j) - m)^2 with m = sum_j l(s_j) / n — the accumulator pixel holds (S, n), the moment buffer M2.
// Chan, Golub & LeVeque's pairwise update ("Updating formulae and a pairwise algorithm for computing sample variances",
// 1979) merges two states without ever forming sum l^2 - n m^2, which in binary32 cancels to noise of the order of
// n 2^-24 m^2: more than the variance itself on the smooth pixels a variance-guided filter cares about.
// The kernels (pt_kernels.hip, rt_amd.hip) and the host's rt_moments_merge call this very function; no translation unit
// contracts a*b+c, so both evaluate the same operations (the policies differ in the rounding of `/` only).
#pragma once
#include <hip/hip_runtime.h>

namespace pt {

#define PT_MOM_HD __host__ __device__ inline

// the luminance of rt_denoise_variance
PT_MOM_HD float moments_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// (nA, SA, M2A) (+) (nB, SB, M2B) -> M2 of the union; the counts are the accumulator's floats (exact integers)
PT_MOM_HD float moments_merge(float nA, float sAr, float sAg, float sAb, float m2A, float nB, float sBr, float sBg, float sBb,
                              float m2B) {
    if (nA == 0.0f) return m2B;
    if (nB == 0.0f) return m2A;
    const float delta = moments_lum(sBr, sBg, sBb) / nB - moments_lum(sAr, sAg, sAb) / nA;
    return m2A + m2B + (delta * delta) * (nA * nB / (nA + nB));
}

}  // namespace pt
