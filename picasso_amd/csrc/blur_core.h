// blur_core.h — the arithmetic of one output sample of the separable blur (csrc/blur.hip), shared with the host-side
// check of it (tests/blur_host_driver.cpp).  scipy.ndimage.correlate1d for symmetric weights, in float64:
//     tmp = line[l] * w[r];   for j = r, r - 1, ..., 1:   tmp += (line[l - j] + line[l + j]) * w[r - j];
// The kernels walk j in chunks staged in LDS and the host walks it in one plain loop; both go through the two functions
// below, one call per term and in the same order, so they round alike.  Build with contraction off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PMI_BLUR_FN __host__ __device__ __forceinline__
#else
#define PMI_BLUR_FN static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pmi {
namespace blur {

PMI_BLUR_FN double centre_term(double centre, double w_r) { return centre * w_r; }

// the term of one j: the samples at l - j (far) and l + j (near), the weight w[r - j]
PMI_BLUR_FN double add_pair(double tmp, double far, double near, double w) { return tmp + (far + near) * w; }

// what leaves a pass: float32 between the axes and at the end of the spatial route; on the direct route the last pass
// multiplies by the scale first
PMI_BLUR_FN float round_out(double tmp, int scale_out, double scale) { return scale_out ? (float)(tmp * scale) : (float)tmp; }

}  // namespace blur
}  // namespace pmi
