// hyper_host.h — the host side the hyperelastic entry points share (icnn.hip, hyper3.hip, field_ops.hip): the network and the analytic
// Isihara model, each for a 2x2 and for a 3x3 F, as an array entry (F[n] -> dP[n], P[n]) and as a field entry (u on a mesh -> dP, P).
// The 2-D and 3-D forms differ in the row widths dim^2 and dim^4 and in the kernel behind them; the checks, their order, their texts
// ("<entry>: <what>") and the device / host-pipeline drivers are written here once. Host code only.
#pragma once

#include "dxo_common.h"
#include "hyper_core.h"
#include "form_host.h"

namespace {

// ---- array entries: dxo_icnn_eval, dxo_icnn3_eval, dxo_isihara, dxo_isihara3 after their own ctx / model-or-params / precision lines.
// `chunk` is the operator's pipeline callback, d_in = {F}, d_out = {dP, P}; device arrays go through it in one piece.
inline int hyper_array_entry(dxo_ctx* ctx, const char* who, int64_t n, int mem, const double* F, double* dP, double* P, int dim,
                             dxo_chunk_launch chunk, void* user, bool stream_once) {
    if (n < 0) return fail_who(ctx, DXO_E_SIZE, who, "n < 0");
    if (mem != DXO_MEM_HOST && mem != DXO_MEM_DEVICE) return fail_who(ctx, DXO_E_MEM, who, "bad mem");
    if (n > 0 && (!F || !dP || !P)) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    const uintptr_t all = (uintptr_t)F | (uintptr_t)dP | (uintptr_t)P;
    if (all & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    if (mem == DXO_MEM_DEVICE && (all & 15u)) return fail_who(ctx, DXO_E_ALIGN, who, "device arrays must be 16-byte aligned");
    if (mem == DXO_MEM_DEVICE) {
        hipStream_t s = dxo_launch_stream(ctx);
        int rc = dxo_device_begin(ctx, s);
        if (rc != DXO_OK) return rc;
        void* d_in[1] = {const_cast<double*>(F)};
        void* d_out[2] = {dP, P};
        rc = chunk(ctx, user, n, d_in, d_out, s);
        if (rc != DXO_OK) return rc;
        return dxo_device_end(ctx, s);
    }
    const size_t row = sizeof(double) * dim * dim;
    std::vector<dxo_span> in = {{F, nullptr, row}};
    std::vector<dxo_span> out = {{nullptr, dP, row * dim * dim}, {nullptr, P, row}};
    return dxo_run_host_pipeline(ctx, n, in, out, chunk, user, 1, nullptr, stream_once);
}

// ---- field entries. The mesh of a `*_field` entry: the 2-D texts carry no entry name (they never did), the 3-D texts do, and `what3`
// says what is 3-D about the entry.
inline int field_check_mesh(dxo_ctx* ctx, const char* who, int dim, const dxo_mesh* mesh, const char* what3) {
    if (dim == 2) {
        if (!mesh) return dxo_fail(ctx, DXO_E_NULL, "mesh is NULL");
        if (mesh->gdim != 2) return dxo_fail(ctx, DXO_E_DIM, "the operator is plane strain / 2-D (Mandel length 4, F 2x2): the mesh must have gdim = 2");
        return DXO_OK;
    }
    if (!mesh) return fail_who(ctx, DXO_E_NULL, who, "mesh is NULL");
    if (mesh->gdim != 3) return fail_who(ctx, DXO_E_DIM, who, what3);
    return DXO_OK;
}

// dxo_icnn_field, dxo_icnn3_field, dxo_isihara_field, dxo_isihara3_field after their ctx / model-or-params lines. The network's precision
// stands between the mesh and mem (the analytic entries pass none). A mesh without cells is DXO_OK before the arrays are looked at: the
// caller returns on `rc != DXO_OK || mesh->num_cells == 0`.
inline int hyper_field_check(dxo_ctx* ctx, const char* who, int dim, const dxo_mesh* mesh, int mem, const double* u, const double* dP,
                             const double* P, int precision = 0) {
    const int rc = field_check_mesh(ctx, who, dim, mesh, "F is 3x3, the mesh must have gdim = 3");
    if (rc != DXO_OK) return rc;
    if (precision != 0 && precision != 1) return fail_who(ctx, DXO_E_OPTION, who, "precision must be 0 (fp32 network) or 1 (fp64)");
    if (mem != DXO_MEM_HOST && mem != DXO_MEM_DEVICE) return fail_who(ctx, DXO_E_MEM, who, "bad mem");
    if (mesh->num_cells == 0) return DXO_OK;
    if (!u || !dP || !P) return fail_who(ctx, DXO_E_NULL, who, "NULL array");
    const uintptr_t all = (uintptr_t)u | (uintptr_t)dP | (uintptr_t)P;
    if (all & 7u) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    if (mem == DXO_MEM_DEVICE && (((uintptr_t)dP | (uintptr_t)P) & 15u)) return fail_who(ctx, DXO_E_ALIGN, who, "device dP, P must be 16-byte aligned");
    return DXO_OK;
}

// ---- the analytic model with F formed in the registers of the kernel that evaluates it (isihara_field, isihara3_field): cells
// [cell0, cell0 + n_cells) of the mesh, u on the device
struct IsiFieldLaunch {
    IsiPrm prm;
    dxo_mesh* mesh;
    const double* d_u;
    int (*launch)(dxo_ctx*, const IsiFieldLaunch&, int64_t cell0, int64_t n_cells, double* dP, double* P, hipStream_t);
    int64_t next_cell = 0;
};

inline int isi_field_chunk(dxo_ctx* ctx, void* user, int64_t n_chunk, void* const*, void* const* d_out, hipStream_t s) {
    IsiFieldLaunch& L = *static_cast<IsiFieldLaunch*>(user);
    const int64_t cell0 = L.next_cell;
    L.next_cell += n_chunk;
    return L.launch(ctx, L, cell0, n_chunk, (double*)d_out[0], (double*)d_out[1], s);
}

// device arrays: one launch over all cells; host arrays: u goes up whole, the cells stream through the pipeline
inline int isi_field_run(dxo_ctx* ctx, IsiFieldLaunch L, int dim, int mem, double* dP, double* P) {
    dxo_mesh* mesh = L.mesh;
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    if (mem == DXO_MEM_DEVICE) {
        hipStream_t s = dxo_launch_stream(ctx);
        int rc = dxo_device_begin(ctx, s);
        if (rc != DXO_OK) return rc;
        rc = L.launch(ctx, L, 0, mesh->num_cells, dP, P, s);
        if (rc != DXO_OK) return rc;
        return dxo_device_end(ctx, s);
    }
    int rc = upload_u(ctx, mesh, L.d_u, mesh->gdim);
    if (rc != DXO_OK) return rc;
    L.d_u = mesh->d_u;
    const size_t row = sizeof(double) * (size_t)mesh->dev.nq * dim * dim;
    std::vector<dxo_span> in;
    std::vector<dxo_span> out = {{nullptr, dP, row * dim * dim}, {nullptr, P, row}};
    return dxo_run_host_pipeline(ctx, mesh->num_cells, in, out, isi_field_chunk, &L, mesh->dev.nq, nullptr, true);
}

}  // namespace
