// csr.h — the CSR pattern of a blocked Lagrange field (dxo_csr_create, assemble.hip), shared by the assembly and the Krylov
// kernels (krylov.hip). Rows node*bs + i of one node hold the same columns; the columns come in runs m*bs + j, j < bs.
#pragma once

#include "dxo_common.h"

// option assemble_chunk_cells = 0: the element matrices of a chunk (of cells, assemble.hip; of facet entities, facet_form.hip) <= 1 GiB
constexpr int64_t DXO_AS_AUTO_SCRATCH_BYTES = (int64_t)1 << 30;

struct dxo_csr {
    const dxo_mesh* mesh = nullptr;
    int bs = 0, nd = 0;
    int64_t n_nodes = 0, n_cells = 0, n_rows = 0, nnz = 0;
    int64_t* d_row_ptr = nullptr;      // [n_rows + 1]
    int32_t* d_col = nullptr;          // [nnz]
    int64_t* d_inc_ptr = nullptr;      // [n_nodes + 1] incidences of a node
    uint32_t* d_inc = nullptr;         // cell * nd + a, ascending cell per node
    uint16_t* d_pos = nullptr;         // [n_cells][nd][nd] column block of b's node in the rows of a's node
    uint8_t* d_mask = nullptr;         // [n_rows] constrained dofs of the last dxo_csr_dirichlet
    double* d_ae = nullptr;            // element-matrix scratch of one chunk
    size_t ae_cap = 0;
    double build_ms = 0.0;
};
