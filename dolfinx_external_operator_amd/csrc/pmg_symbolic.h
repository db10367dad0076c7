// pmg_symbolic.h — the symbolic part of dxo_pmg_create (pmg.hip): plain host C++, no HIP, so that it can be built and run on its own
// (tests/helpers/pmg_symbolic_main.cpp, under AddressSanitizer and UBSan).
//   pmg_check_transfer  the checks of a dxo_amg_transfer, those of dxo_amg_create_transfer with its error codes but for the stagnation
//                       rule of the multigrid's coarsening, which says nothing about a transfer (n_coarse above n_nodes: DXO_E_SIZE)
//   pmg_build_tables    p_diag [block][bs] = w_iv keep(i, c) keep(coarse_to_fine[v], c), the transposed incidence of P (coarse node ->
//                       its blocks, fine nodes ascending) and the constrained dofs of the coarse space, ascending
#pragma once

#include "dxo.h"

#include <cmath>
#include <cstdint>
#include <vector>

struct pmg_tables {
    std::vector<int64_t> p_ptr;        // [n_nodes + 1]
    std::vector<int32_t> p_col;        // [p_blocks] coarse node
    std::vector<double> p_diag;        // [p_blocks][bs]
    std::vector<int64_t> pt_ptr;       // [n_coarse + 1]
    std::vector<int64_t> pt_blk;       // [p_blocks] position in p_col / p_diag
    std::vector<int32_t> pt_row;       // [p_blocks] its fine node
    std::vector<int32_t> c_bc;         // constrained dofs of the coarse space
};

// DXO_OK, or the code of the first rule the transfer breaks with *what naming it. The arrays are not NULL (checked by the caller)
inline int pmg_check_transfer(int64_t n, const dxo_amg_transfer& w, const char** what) {
    const int64_t nc = w.n_coarse;
    auto fail = [&](int code, const char* text) {
        *what = text;
        return code;
    };
    if (nc < 1 || nc > n) return fail(DXO_E_SIZE, "n_coarse must be at least 1 and at most n_nodes");
    if (w.ptr[0] != 0) return fail(DXO_E_SIZE, "ptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i) {
        if (w.ptr[i + 1] <= w.ptr[i]) return fail(DXO_E_SIZE, "every node needs at least one entry (ptr must increase)");
        for (int64_t e = w.ptr[i]; e < w.ptr[i + 1]; ++e) {
            if (w.col[e] < 0 || w.col[e] >= nc) return fail(DXO_E_SIZE, "a column lies outside [0, n_coarse)");
            if (e > w.ptr[i] && w.col[e] <= w.col[e - 1]) return fail(DXO_E_OPTION, "the columns of a row must ascend");
            if (!std::isfinite(w.w[e])) return fail(DXO_E_OPTION, "a weight is not finite");
        }
    }
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t v = 0; v < nc; ++v) {
        const int64_t i = w.coarse_to_fine[v];
        if (i < 0 || i >= n) return fail(DXO_E_SIZE, "coarse_to_fine lies outside [0, n_nodes)");
        if (seen[(size_t)i]) return fail(DXO_E_OPTION, "coarse_to_fine names a node twice");
        seen[(size_t)i] = 1;
        const int64_t e = w.ptr[i];
        if (w.ptr[i + 1] != e + 1 || w.col[e] != v || w.w[e] != 1.0) return fail(DXO_E_OPTION, "the row of coarse_to_fine[v] must be the single entry (v, 1)");
    }
    return DXO_OK;
}

// the tables of a checked transfer; mask [n * bs]: 1 for a constrained fine dof
inline void pmg_build_tables(int64_t n, int bs, const dxo_amg_transfer& w, const std::vector<uint8_t>& mask, pmg_tables& t) {
    const int64_t nc = w.n_coarse, pb = w.ptr[n];
    t.p_ptr.assign(w.ptr, w.ptr + n + 1);
    t.p_col.assign(w.col, w.col + pb);
    t.p_diag.resize((size_t)(pb * bs));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = w.ptr[i]; e < w.ptr[i + 1]; ++e) {
            const int64_t f = w.coarse_to_fine[w.col[e]];
            for (int c = 0; c < bs; ++c)
                t.p_diag[(size_t)(e * bs + c)] = w.w[e] * (mask[(size_t)(i * bs + c)] ? 0.0 : 1.0) * (mask[(size_t)(f * bs + c)] ? 0.0 : 1.0);
        }
    // the transposed incidence: a counting sort of the blocks by coarse node over the rows in ascending order
    t.pt_ptr.assign((size_t)nc + 1, 0);
    t.pt_blk.resize((size_t)pb);
    t.pt_row.resize((size_t)pb);
    for (int64_t e = 0; e < pb; ++e) ++t.pt_ptr[(size_t)w.col[e] + 1];
    for (int64_t v = 0; v < nc; ++v) t.pt_ptr[(size_t)v + 1] += t.pt_ptr[(size_t)v];
    std::vector<int64_t> at(t.pt_ptr.begin(), t.pt_ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = w.ptr[i]; e < w.ptr[i + 1]; ++e) {
            const int64_t q = at[(size_t)w.col[e]]++;
            t.pt_blk[(size_t)q] = e;
            t.pt_row[(size_t)q] = (int32_t)i;
        }
    // (v, c) is constrained iff (coarse_to_fine[v], c) is
    t.c_bc.clear();
    for (int64_t v = 0; v < nc; ++v)
        for (int c = 0; c < bs; ++c)
            if (mask[(size_t)((int64_t)w.coarse_to_fine[v] * bs + c)]) t.c_bc.push_back((int32_t)(v * bs + c));
}
