// form_host.h — the host side every form file shares: from a mesh, an operand kind and a block size to a launch. The dispatchers from
// run-time shapes to template arguments (with_int and the lists built on it), the table of bilinear pairs, the two grid forms, the
// grow-only device buffers and uploads, the chunk rule and chunk loop of the two-pass assemblies, the slab of the facet-table setters, the
// transposed incidence, and the staging of host arrays around a launch. Host code only: no kernel is instantiated by including it.
#pragma once

#include "operand_core.h"

#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <type_traits>
#include <vector>

// from a run-time value to a compile-time one: f(int_c<N>) for the entry N of the list that equals v, miss(v) for none. A list is the
// set of instantiations of its caller, so a kernel's argument list is written once
template <int N>
using int_c = std::integral_constant<int, N>;

template <int... Ns, class F, class Miss>
void with_int(int v, F&& f, Miss&& miss) {
    if (!((v == Ns && (f(int_c<Ns>{}), true)) || ...)) miss(v);
}

// the geometric dimensions: f(int_c<2>) or f(int_c<3>) and DXO_OK; DXO_E_DIM and no call for any other
template <class F>
int with_gdim(int gdim, F&& f) {
    int rc = DXO_OK;
    with_int<2, 3>(gdim, f, [&](int) { rc = DXO_E_DIM; });
    return rc;
}

// f(int_c<G>, int_c<BS>) for the dense shapes (2,1), (2,2), (3,1), (3,3); its result, or DXO_E_DIM for any other shape
template <class F>
int with_form_shape(int gdim, int bs, F&& f) {
    int rc = DXO_E_DIM;
    auto miss = [](int) {};
    if (gdim == 2) with_int<1, 2>(bs, [&](auto BS) { rc = f(int_c<2>{}, BS); }, miss);
    else if (gdim == 3) with_int<1, 3>(bs, [&](auto BS) { rc = f(int_c<3>{}, BS); }, miss);
    return rc;
}

inline bool op_is_nonlinear(int kind) { return kind == DXO_OPERAND_CAUCHY_GREEN || kind == DXO_OPERAND_I1 || kind == DXO_OPERAND_DETF; }

// f(int_c<KIND>) and DXO_OK; DXO_E_OPTION for a kind outside the list (LINEAR_ONLY: the kinds with an adjoint). The kinds of a vector
// field (eps, F, div, C, I1, det F) are instantiated for BS == G alone and answer DXO_E_DIM otherwise
template <int G, int BS, bool LINEAR_ONLY, class F>
int with_operand_kind(int kind, F&& f) {
    int rc = DXO_E_OPTION;
    auto any = [&](auto K) { f(K); rc = DXO_OK; };
    auto vec = [&](auto K) {
        if constexpr (BS == G) any(K);
        else rc = DXO_E_DIM;
    };
    auto miss = [](int) {};
    with_int<DXO_OPERAND_VALUE, DXO_OPERAND_GRAD, DXO_OPERAND_VALUE_GRAD>(kind, any, [&](int) {
        with_int<DXO_OPERAND_EPS_MANDEL, DXO_OPERAND_DEFGRAD, DXO_OPERAND_DIV>(kind, vec, [&](int) {
            if constexpr (!LINEAR_ONLY) with_int<DXO_OPERAND_CAUCHY_GREEN, DXO_OPERAND_I1, DXO_OPERAND_DETF>(kind, vec, miss);
        });
    });
    return rc;
}

// the block sizes of a node sum: 1, and gdim = 2, 3
template <class F>
void with_node_bs(int bs, F&& f) { with_int<1, 2, 3>(bs, f, [](int) {}); }

// the supported bilinear pairs (include/dxo.h): f(int_c<BS>, int_c<TEST>, int_c<TRIAL>) and true, or false
template <int G, class F>
bool with_bilinear_pair(int bs, int test, int trial, F&& f) {
    constexpr int V = DXO_OPERAND_VALUE, GR = DXO_OPERAND_GRAD, VG = DXO_OPERAND_VALUE_GRAD, EPS = DXO_OPERAND_EPS_MANDEL;
    auto is = [&](auto BS, auto T, auto R) { return bs == BS && test == T && trial == R && (f(BS, T, R), true); };
    return is(int_c<G>{}, int_c<GR>{}, int_c<GR>{}) || is(int_c<G>{}, int_c<EPS>{}, int_c<EPS>{}) || is(int_c<1>{}, int_c<GR>{}, int_c<VG>{}) ||
           is(int_c<1>{}, int_c<GR>{}, int_c<GR>{}) || is(int_c<1>{}, int_c<V>{}, int_c<V>{}) || is(int_c<1>{}, int_c<VG>{}, int_c<VG>{});
}

// the opening of dxo_bilinear_apply / _diagonal / _assemble: the nonlinear kinds refused, DEFGRAD taken as its linearisation GRAD, the
// pair looked up (ops = select(int_c<G>, int_c<BS>, int_c<TEST>, int_c<TRIAL>)), the quadrature weights present
template <class Ops, class Select>
int bilinear_pair_check(dxo_ctx* ctx, const char* who, const dxo_mesh* mesh, int test, int trial, int bs, Ops& ops, Select select) {
    if (op_is_nonlinear(test) || op_is_nonlinear(trial))
        return fail_who(ctx, DXO_E_OPTION, who, "a nonlinear operand (C, I1, det F) has no bilinear form — pass its linearisation's block");
    const int t = test == DXO_OPERAND_DEFGRAD ? DXO_OPERAND_GRAD : test, r = trial == DXO_OPERAND_DEFGRAD ? DXO_OPERAND_GRAD : trial;
    bool found = false;
    if ((test != DXO_OPERAND_DEFGRAD && trial != DXO_OPERAND_DEFGRAD) || bs == mesh->gdim)
        with_gdim(mesh->gdim, [&](auto G) {
            found = with_bilinear_pair<G>(bs, t, r, [&](auto BS, auto T, auto R) { ops = select(G, BS, T, R); });
        });
    if (!found) {
        char msg[320];
        std::snprintf(msg, sizeof msg, "%s: unsupported pair (test kind %d, trial kind %d, bs %d) on gdim %d: bs = gdim takes (grad|F, grad|F) and "
                      "(eps, eps); bs = 1 takes (grad, value_grad), (grad, grad), (value, value), (value_grad, value_grad)", who, test, trial, bs, mesh->gdim);
        return dxo_fail(ctx, DXO_E_OPTION, msg);
    }
    if (!mesh->d_wq) return fail_who(ctx, DXO_E_OPTION, who, "quadrature weights not set (dxo_mesh_set_weights)");
    return DXO_OK;
}

// grid of the persistent element kernels: one workgroup (four waves) per four wave groups, at most blocks_per_cu per compute unit (option
// "wave_group_blocks" > 0: at most that many; a cell's result does not depend on which wave forms it), whole rounds over the 8 XCDs
// (xcd_group_walk)
inline int64_t wave_groups(const OperandDev& v, int64_t n_cells) { return (n_cells + v.cells_per_wave - 1) / v.cells_per_wave; }
inline int wave_group_grid(const dxo_ctx* ctx, int64_t n_groups, int blocks_per_cu) {
    int64_t blocks = (n_groups + 3) / 4;
    const int64_t cap = ctx->wave_group_blocks > 0 ? ctx->wave_group_blocks : (int64_t)ctx->compute_units * blocks_per_cu;
    if (blocks > cap) blocks = cap;
    return (int)((blocks + 7) / 8 * 8);
}

// grid of the grid-stride kernels: ceil(work / per_block) workgroups, at least 1, at most blocks_per_cu per compute unit
inline int capped_grid(const dxo_ctx* ctx, int64_t work, int64_t per_block, int blocks_per_cu) {
    int64_t blocks = (work + per_block - 1) / per_block;
    const int64_t cap = (int64_t)ctx->compute_units * blocks_per_cu;
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : (int)blocks;
}

// grow-only device buffer: at least `bytes` at *p, its capacity at *cap. On failure *p is null and the error is returned, not reported
inline hipError_t device_buf_try(void** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return hipSuccess;
    hipError_t e = *p ? hipFree(*p) : hipSuccess;
    *p = nullptr;
    *cap = 0;
    if (e == hipSuccess) e = hipMalloc(p, bytes);
    if (e == hipSuccess) *cap = bytes;
    return e;
}

inline int device_buf(dxo_ctx* ctx, void** p, size_t* cap, size_t bytes) {
    DXO_HIP(ctx, device_buf_try(p, cap, bytes));
    return DXO_OK;
}

// option assemble_chunk_cells = 0: the element matrices of a chunk (of cells, assemble.hip; of facet entities, facet_form.hip) <= 1 GiB
constexpr int64_t DXO_AS_AUTO_SCRATCH_BYTES = (int64_t)1 << 30;

// entities per chunk of a two-pass assembly of n entities with ent_bytes of element matrix each, within [1, n]
inline int64_t assemble_chunk(const dxo_ctx* ctx, size_t ent_bytes, int64_t n) {
    const int64_t chunk = ctx->assemble_chunk_cells > 0 ? ctx->assemble_chunk_cells : DXO_AS_AUTO_SCRATCH_BYTES / (int64_t)ent_bytes;
    return std::max<int64_t>(1, std::min(chunk, n));
}

// the two passes of an assembly over n entities, chunk by chunk: the grow-only scratch (*ae, *cap) takes one chunk's element matrices (the
// first call, or a larger chunk, allocates), begin() opens the launches, then elem(e0, e1) and rows(e0, e1) per chunk [e0, e1)
template <class Begin, class Elem, class Rows>
int assemble_two_pass(dxo_ctx* ctx, int64_t n, size_t ent_bytes, double** ae, size_t* cap, Begin&& begin, Elem&& elem, Rows&& rows) {
    const int64_t chunk = assemble_chunk(ctx, ent_bytes, n);
    int rc = device_buf(ctx, (void**)ae, cap, (size_t)chunk * ent_bytes);
    if (rc == DXO_OK) rc = begin();
    if (rc != DXO_OK) return rc;
    for (int64_t e0 = 0; e0 < n; e0 += chunk) {
        const int64_t e1 = std::min(n, e0 + chunk);
        elem(e0, e1);
        rows(e0, e1);
    }
    return DXO_OK;
}

// a new device slab holding the host arrays `parts` (pointer, doubles) back to back, in place of *slab. The device is drained first: a
// queued launch may still read the old slab. The caller keeps the slab's dimensions at zero until this returns DXO_OK
struct host_part {
    const double* p;
    size_t n;
};
inline int upload_slab(dxo_ctx* ctx, double** slab, const host_part (&parts)[3]) {
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    DXO_HIP(ctx, hipDeviceSynchronize());
    if (*slab) DXO_HIP(ctx, hipFree(*slab));
    *slab = nullptr;
    DXO_HIP(ctx, hipMalloc((void**)slab, (parts[0].n + parts[1].n + parts[2].n) * sizeof(double)));
    size_t at = 0;
    for (const host_part& h : parts) {
        DXO_HIP(ctx, hipMemcpy(*slab + at, h.p, h.n * sizeof(double), hipMemcpyHostToDevice));
        at += h.n;
    }
    return DXO_OK;
}

// the dof vector of a host caller (`components` values per field node) into the mesh's grow-only staging buffer d_u, whole
static inline int upload_u(dxo_ctx* ctx, dxo_mesh* mesh, const double* u, int components) {
    const size_t ub = (size_t)mesh->num_field_nodes * components * sizeof(double);
    const int rc = device_buf(ctx, (void**)&mesh->d_u, &mesh->u_cap, ub);
    if (rc != DXO_OK) return rc;
    DXO_HIP(ctx, hipMemcpy(mesh->d_u, u, ub, hipMemcpyHostToDevice));
    return DXO_OK;
}

// a new device array with the n entries of src, extra_bytes more allocated behind them (kernels that read whole vectors past the end)
template <class T>
int to_device(dxo_ctx* ctx, T** dst, const T* src, size_t n, size_t extra_bytes = 0) {
    DXO_HIP(ctx, hipMalloc((void**)dst, n * sizeof(T) + extra_bytes));
    if (n) DXO_HIP(ctx, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return DXO_OK;
}

template <class T>
int to_device(dxo_ctx* ctx, T** dst, const std::vector<T>& src, size_t extra_bytes = 0) {
    return to_device(ctx, dst, src.data(), src.size(), extra_bytes);
}

inline void free_all(std::initializer_list<void*> ptrs) {
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
}

// the transposed incidence of n_entries entries over n_nodes nodes: entry e belongs to node_of(e); ent[ptr[n] .. ptr[n + 1]) holds
// value_of(e) of the node's entries in ascending e (a fixed order per node). false if a node lies outside [0, n_nodes)
template <class NodeOf, class ValueOf>
bool transpose_incidence(int64_t n_entries, int64_t n_nodes, NodeOf node_of, ValueOf value_of, std::vector<int64_t>& ptr,
                         std::vector<uint32_t>& ent) {
    ptr.assign((size_t)n_nodes + 1, 0);
    for (int64_t e = 0; e < n_entries; ++e) {
        const int64_t n = node_of(e);
        if (n < 0 || n >= n_nodes) return false;
        ++ptr[(size_t)n + 1];
    }
    for (int64_t n = 0; n < n_nodes; ++n) ptr[(size_t)n + 1] += ptr[(size_t)n];
    ent.resize((size_t)n_entries);
    std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t e = 0; e < n_entries; ++e) ent[(size_t)fill[(size_t)node_of(e)]++] = (uint32_t)value_of(e);
    return true;
}

// ---- host arrays around a launch (mem == DXO_MEM_HOST): entity lists checked, inputs staged in the mesh's grow-only buffers, the
// output copied back
inline bool cells_ok(const dxo_mesh* m, const int32_t* cells, int64_t n) {
    for (int64_t i = 0; cells && i < n; ++i)
        if (cells[i] < 0 || cells[i] >= m->num_cells) return false;
    return true;
}

inline bool facet_entities_ok(const dxo_mesh* m, const int32_t* ents, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (ents[2 * i] < 0 || ents[2 * i] >= m->num_cells || ents[2 * i + 1] < 0 || ents[2 * i + 1] >= m->n_local_facets) return false;
    return true;
}

// n entries of `host` into the buffer (*buf, *cap) on the stream; *dev = the device copy
template <class T>
int stage_in(dxo_ctx* ctx, T** buf, size_t* cap, const T* host, size_t n, hipStream_t s, const T** dev) {
    const int rc = device_buf(ctx, (void**)buf, cap, n * sizeof(T));
    if (rc != DXO_OK) return rc;
    DXO_HIP(ctx, hipMemcpyAsync(*buf, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    *dev = *buf;
    return DXO_OK;
}

// the staged output (the mesh's d_out) back into the caller's array; waits for the stream
inline int stage_out(dxo_ctx* ctx, double* host, const double* dev, size_t bytes, hipStream_t s) {
    DXO_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    DXO_HIP(ctx, hipStreamSynchronize(s));
    return DXO_OK;
}
