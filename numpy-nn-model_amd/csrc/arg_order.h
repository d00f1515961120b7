// arg_order.h -- the one (value, index) order behind every index-valued reduction of the library: np.argmax's for embedding.hip's
// argmax kernels, and its mirror image, np.argmin's, for the nearest-code search of vector_quantize.hip.  Index results are bit-exact
// by construction: a pure comparison network, (value, index) pairs ordered by (value desc, index asc).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nnhip {

struct ArgBest {
    float v;
    int32_t i;
};
// np.argmax: is (v, i) a better maximum than (bv, bi)?
__device__ __forceinline__ bool arg_better(float v, int32_t i, float bv, int32_t bi) {
    const bool vn = v != v, bn = bv != bv;
    // a NaN beats any number | two NaNs, or a tie: the earlier index | else the larger value (false as soon as a NaN is involved).
    // Bitwise on purpose: as `if`s this became three branches per candidate inside the nearest-code search's MFMA loop.
    return (vn & !bn) | (((vn & bn) | (v == bv)) & (i < bi)) | (v > bv);
}
// np.argmin: the same order on the negated values (a negation is exact, keeps a NaN a NaN and is a source modifier on the VALU)
__device__ __forceinline__ bool arg_better_min(float v, int32_t i, float bv, int32_t bi) { return arg_better(-v, i, -bv, bi); }

}  // namespace nnhip
