// csr.h — the CSR pattern of a blocked Lagrange field (dxo_csr_create, assemble.hip), shared by the assembly and the Krylov
// kernels (krylov.hip). Rows node*bs + i of one node hold the same columns; the columns come in runs m*bs + j, j < bs.
// And assemble_rows, the row pass both assemblies on the pattern end with (assemble.hip over cells, facet_form.hip over facet entities).
#pragma once

#include "dxo_common.h"

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
    uint16_t* d_mirror = nullptr;      // [nnz / bs^2] transpose.hip: position of a block's row node in the rows of its column node
    int mirror_state = 0;              // 0: not built yet, 1: built, -1: built and the pattern found not structurally symmetric
    double* d_ae = nullptr;            // element-matrix scratch of one chunk
    size_t ae_cap = 0;
    double build_ms = 0.0;
};

namespace {

// the row sets of assemble_rows: n nodes, node t with the incidences inc[ptr[t] .. ptr[t + 1]) = entity * nd + a in ascending entity order;
// row(r, t, i) is the pattern's row of the set's row r = t * BS + i.
// Every node of the pattern, the entities its cells: the set's rows are the pattern's, an incidence is the entry's place in `pos`
struct CellRows {
    int64_t n;
    const int64_t* ptr;
    const uint32_t* inc;
    template <int BS>
    __device__ int64_t row(int64_t r, int64_t, int) const { return r; }
    __device__ int64_t pos_entry(uint32_t ent, int64_t, int, int) const { return ent; }
};
// the touched nodes of a facet set, the entities its (cell, local facet) pairs: `pos` is indexed through the entity's cell
struct FacetRows {
    int64_t n;
    const int64_t* ptr;
    const uint32_t* inc;
    const int32_t* tnode;      // [n] the nodes, ascending
    const int32_t* ents;       // [.][2]
    template <int BS>
    __device__ int64_t row(int64_t, int64_t t, int i) const { return (int64_t)tnode[t] * BS + i; }
    __device__ int64_t pos_entry(uint32_t, int64_t e, int a, int nd) const { return (int64_t)ents[2 * e] * nd + a; }
};

// pass 2 of an assembly: one thread per row (node, component i) of the row set adds the entries of the chunk's entities [e_begin, e_end),
// element matrices ae[e - e_begin][a*BS + i][b*BS + j], in ascending entity order (the fixed order of the incidences)
template <int BS, int BLOCK, class Rows>
__global__ __launch_bounds__(BLOCK) void assemble_rows(Rows rows, int nd, const int64_t* __restrict__ row_ptr, const uint16_t* __restrict__ pos,
                                                       const double* __restrict__ ae, int64_t e_begin, int64_t e_end,
                                                       double* __restrict__ values) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int ndb = nd * BS;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows.n * BS; r += stride) {
        const int64_t t = r / BS;
        const int i = (int)(r - t * BS);
        const int64_t j0 = rows.ptr[t], j1 = rows.ptr[t + 1];
        if (j0 == j1 || (int64_t)(rows.inc[j1 - 1] / nd) < e_begin || (int64_t)(rows.inc[j0] / nd) >= e_end) continue;
        double* row = values + row_ptr[rows.template row<BS>(r, t, i)];
        for (int64_t j = j0; j < j1; ++j) {
            const uint32_t ent = rows.inc[j];
            const int64_t e = ent / nd;
            if (e < e_begin) continue;
            if (e >= e_end) break;
            const int a = (int)(ent - e * nd);
            const double* src = ae + ((e - e_begin) * ndb + (int64_t)a * BS + i) * ndb;
            const uint16_t* pp = pos + rows.pos_entry(ent, e, a, nd) * nd;
            for (int b = 0; b < nd; ++b) {
                double* dst = row + (int64_t)pp[b] * BS;
#pragma unroll
                for (int jj = 0; jj < BS; ++jj) dst[jj] += src[b * BS + jj];
            }
        }
    }
}

}  // namespace
