// krylov_internal.h — launchers shared between krylov.hip and amg.hip (device pointers, explicit stream, no locking, no event bracket).
#pragma once

#include "csr.h"

// the closed-form inverse of a diagonal block (bs <= 3) and its singularity test, for dxo_csr_block_jacobi (krylov.hip) and the lumped
// diagonal blocks of the filtered prolongator smoothing (amg.hip)
template <int BS>
__device__ __forceinline__ bool invert_block(const double (&a)[BS][BS], double (&b)[BS][BS]) {
    double had = 1.0;
#pragma unroll
    for (int i = 0; i < BS; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < BS; ++j) s += a[i][j] * a[i][j];
        had *= sqrt(s);
    }
    double det;
    if constexpr (BS == 1) {
        det = a[0][0];
        b[0][0] = 1.0 / det;
    } else if constexpr (BS == 2) {
        det = a[0][0] * a[1][1] - a[0][1] * a[1][0];
        const double id = 1.0 / det;
        b[0][0] = a[1][1] * id;
        b[0][1] = -a[0][1] * id;
        b[1][0] = -a[1][0] * id;
        b[1][1] = a[0][0] * id;
    } else {
        const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1];
        const double c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2];
        const double c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
        det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02;
        const double id = 1.0 / det;
        b[0][0] = c00 * id;
        b[1][0] = c01 * id;
        b[2][0] = c02 * id;
        b[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * id;
        b[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * id;
        b[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * id;
        b[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * id;
        b[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * id;
        b[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * id;
    }
    return fabs(det) > 1e-14 * had;     // false for a zero, NaN or nearly singular block
}

// krylov.hip: the block-inverse kernel of dxo_csr_block_jacobi without its wait; a singular block raises flag[0]
void dxo_kr_bj_setup_launch(const dxo_csr* csr, const double* values, double* inv, int* flag, hipStream_t s);

// amg.hip: the checks of a DXO_PC_AMG preconditioner against the operator, and one V-cycle z = V(r) on the stream
int dxo_amg_pc_check(dxo_ctx* ctx, const char* who, const dxo_amg* amg, const dxo_csr* op_csr, int bs, int64_t n);
void dxo_amg_cycle(dxo_ctx* ctx, dxo_amg* amg, const double* r, double* z, hipStream_t s);
