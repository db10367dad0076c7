// operand_coef.h — the operand slots of a unit dof as compile-time coefficients, shared by the matrix-free bilinear kernels
// (bilinear.h) and the sparse assembly (assemble.hip).
#pragma once

#include "dxo.h"

namespace {

// d(slot r of operand KIND) / d z for the unit dof of component i, z = 0: the basis function's value, z = 1 + j: its derivative along
// x_j. Compile-time constants once the callers' loops are unrolled: the zero terms are never formed.
template <int G, int BS, int KIND>
__device__ __forceinline__ constexpr double op_coef(int r, int i, int z) {
    if constexpr (KIND == DXO_OPERAND_VALUE) return (r == i && z == 0) ? 1.0 : 0.0;
    else if constexpr (KIND == DXO_OPERAND_GRAD) return (z > 0 && r == i * G + z - 1) ? 1.0 : 0.0;
    else if constexpr (KIND == DXO_OPERAND_VALUE_GRAD) return ((z == 0 && r == i) || (z > 0 && r == BS + i * G + z - 1)) ? 1.0 : 0.0;
    else {   // EPS_MANDEL (BS == G): e_i = g_ii, e_m(i,j) = (g_ij + g_ji) / sqrt2
        if (z == 0) return 0.0;
        const int j = z - 1;
        if (i == j) return r == i ? 1.0 : 0.0;
        return r == (G == 2 ? 3 : i + j + 2) ? 0.70710678118654752440 : 0.0;
    }
}

template <int KIND>
constexpr bool op_has_value() { return KIND == DXO_OPERAND_VALUE || KIND == DXO_OPERAND_VALUE_GRAD; }
template <int KIND>
constexpr bool op_has_grad() { return KIND != DXO_OPERAND_VALUE; }

}  // namespace
