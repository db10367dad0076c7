// krylov_internal.h — launchers shared between krylov.hip and amg.hip (device pointers, explicit stream, no locking, no event bracket).
#pragma once

#include "csr.h"

// krylov.hip: the block-inverse kernel of dxo_csr_block_jacobi without its wait; a singular block raises flag[0]
void dxo_kr_bj_setup_launch(const dxo_csr* csr, const double* values, double* inv, int* flag, hipStream_t s);

// amg.hip: the checks of a DXO_PC_AMG preconditioner against the operator, and one V-cycle z = V(r) on the stream
int dxo_amg_pc_check(dxo_ctx* ctx, const char* who, const dxo_amg* amg, const dxo_csr* op_csr, int bs, int64_t n);
void dxo_amg_cycle(dxo_ctx* ctx, dxo_amg* amg, const double* r, double* z, hipStream_t s);
