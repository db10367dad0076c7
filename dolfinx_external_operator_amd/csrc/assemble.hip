// assemble.hip — sparse assembly of a bilinear form between two linear operand kinds of one field with a per-point block C_q
// (dxo_csr_* / dxo_bilinear_assemble / dxo_csr_dirichlet): the assembled Jacobian the reference's demos hand to their LU solve,
// assemble_matrix(J_replaced, bcs) (demo_plasticity_von_mises.py:422-434, demo_hyperelasticity.py:560-573,
// demo_nonlinear_heat_equation_part2.py:313-335).
//   values[(a,i),(b,j)] (+)= sum_cells sum_q w_q |det J_q| (B_test,q^T C_q B_trial,q)_((a,i),(b,j))
// The pairs and the C layout are those of dxo_bilinear_apply (bilinear.h).
//
// Pattern (dxo_csr_create, host C++ once per mesh and block size): rows and columns are the blocked dofs node*bs + i; row (n, i)
// holds, for every node m that shares a cell with n (n itself included), the bs columns m*bs + j, sorted ascending. Alongside it,
// per (cell, local node a, local node b), the index of b's node among the sorted neighbours of a's node (`pos`, uint16): the
// column block of the entry in a's rows. And the node -> (cell, a) incidences in ascending cell order (the transposed dofmap).
//
// Values (dxo_bilinear_assemble), default form: TWO PASSES per chunk of cells, no atomics, bit-reproducible.
//   pass 1, assemble_elem: a workgroup owns `cpb` consecutive cells. Phase 1, thread = (cell, point): J^-1, |det J| and the
//     point's block M[i][j][z1][z2] = w|det J| sum_rc coef_test(r, i, z1) C[r][c] coef_trial(c, j, z2) pulled back to
//     reference derivatives (z = (phi, grad phi); the zero coefficients are compile-time and never formed), parked in LDS.
//     Phase 2, thread = (cell, a, b): the BS x BS block A[(a,i),(b,j)] = sum_q z_a,q^T M_q[i][j] z_b,q from the element
//     tables in LDS, written to the chunk's scratch ae[cell][a*BS + i][b*BS + j].
//   pass 2, assemble_rows<.., CellRows> (csr.h, the row pass facet_form.hip shares): one thread per row adds the row's entries of
//     the chunk's cells in ascending cell order (the fixed order of the incidences). Every value is therefore the same chain of
//     additions whatever the chunk size (option "assemble_chunk_cells"): chunk k + 1 continues the chains chunk k left in `values`.
// Option "adjoint_atomics" = 1: pass 1 adds its blocks straight into `values` with fp64 atomics (one launch, no scratch,
// reproducible to rounding only). Option "consumer_overwrite" = 1 clears `values` first (SET instead of accumulate).
#include "csr.h"
#include "dxo_common.h"
#include "form_host.h"
#include "operand_coef.h"

#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include <algorithm>
#include <chrono>
#include <cstdio>

#ifndef DXO_AS_BLOCKS_PER_CU
#define DXO_AS_BLOCKS_PER_CU 8
#endif
#ifndef DXO_AS_BLOCK
#define DXO_AS_BLOCK 256
#endif

namespace {

template <int G, int BS, int TEST, int TRIAL>
struct AsShape {
    static constexpr int DT = OperandShape<G, BS, TEST>::D, DR = OperandShape<G, BS, TRIAL>::D;
    static constexpr int Z0 = (op_has_value<TEST>() || op_has_value<TRIAL>()) ? 0 : 1;   // z = 0 (the value) only where a kind has it
    static constexpr int NZ = G + 1 - Z0;
    static constexpr int PS = (BS * BS * NZ * NZ) | 1;      // parked doubles per point: odd stride (bank spread across cells)
};

// pass 1 (see the head of the file). ae == nullptr: atomics into values through row_ptr / pos.
template <int G, int BS, int TEST, int TRIAL>
__global__ __launch_bounds__(DXO_AS_BLOCK) void assemble_elem(OperandDev m, const double* __restrict__ wq, const double* __restrict__ C,
                                                              int64_t c_begin, int64_t c_end, int cpb, double* __restrict__ ae,
                                                              const int64_t* __restrict__ row_ptr, const uint16_t* __restrict__ pos,
                                                              double* __restrict__ values) {
    using S = AsShape<G, BS, TEST, TRIAL>;
    constexpr int DT = S::DT, DR = S::DR, Z0 = S::Z0, NZ = S::NZ, PS = S::PS;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<G>(m, tab);
    const OperandLayout<G> L(m);
    const int nd = m.ndofs, nq = m.nq, ng = m.ngeom, sx = L.sx;
    double* X = lds + m.table_doubles;                  // [cpb][sx] vertex coordinates
    double* Ms = X + ((cpb * sx + 1) & ~1);             // [cpb * nq][PS] parked point blocks
    const int ndb = nd * BS;
    const int64_t n_cells = c_end - c_begin;
    const int64_t n_groups = (n_cells + cpb - 1) / cpb;
    __syncthreads();
    for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int64_t c0 = c_begin + grp * cpb;
        const int ncell = (c_end - c0 < cpb) ? (int)(c_end - c0) : cpb;
        for (int idx = threadIdx.x; idx < ncell * ng; idx += blockDim.x) {
            const int c = idx / ng, v = idx - c * ng;
            const int64_t node = m.geom_dofmap[(c0 + c) * ng + v];
#pragma unroll
            for (int j = 0; j < G; ++j) X[c * sx + v * G + j] = m.x[node * G + j];
        }
        __syncthreads();
        // phase 1: thread = (cell, point)
        for (int p = threadIdx.x; p < ncell * nq; p += blockDim.x) {
            const int c = p / nq, q = p - c * nq;
            const double* dpsi = tab + L.o_dpsi + q * L.sdpsi;
            const double* Xc = X + c * sx;
            double J[G][G], K[G][G];
#pragma unroll
            for (int j = 0; j < G; ++j)
#pragma unroll
                for (int k = 0; k < G; ++k) J[j][k] = 0.0;
            for (int v = 0; v < ng; ++v)
#pragma unroll
                for (int j = 0; j < G; ++j)
#pragma unroll
                    for (int k = 0; k < G; ++k) J[j][k] += Xc[v * G + j] * dpsi[v * G + k];
            const double scale = wq[q] * fabs(invert<G>(J, K));
            const double* R = C + ((c0 + c) * nq + q) * (int64_t)(DT * DR);
            double* P = Ms + p * PS;
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int jj = 0; jj < BS; ++jj) {
                    // M[z1][z2] in physical derivatives, then P^T M P with P = diag(1, K^T): reference derivatives
                    double M[NZ][NZ];
#pragma unroll
                    for (int z1 = 0; z1 < NZ; ++z1)
#pragma unroll
                        for (int z2 = 0; z2 < NZ; ++z2) {
                            double acc = 0.0;
#pragma unroll
                            for (int r = 0; r < DT; ++r) {
                                const double a = op_coef<G, BS, TEST>(r, i, z1 + Z0);
                                if (a == 0.0) continue;
#pragma unroll
                                for (int cc = 0; cc < DR; ++cc) {
                                    const double b = op_coef<G, BS, TRIAL>(cc, jj, z2 + Z0);
                                    if (b == 0.0) continue;
                                    acc += (a * b) * R[r * DR + cc];
                                }
                            }
                            M[z1][z2] = acc;
                        }
                    double KM[NZ][NZ];
#pragma unroll
                    for (int a = 0; a < NZ; ++a)
#pragma unroll
                        for (int z2 = 0; z2 < NZ; ++z2) {
                            if (a + Z0 == 0) { KM[a][z2] = M[a][z2]; continue; }
                            const int k = a + Z0 - 1;
                            double s = 0.0;
#pragma unroll
                            for (int j = 0; j < G; ++j) s += K[k][j] * M[1 + j - Z0][z2];
                            KM[a][z2] = s;
                        }
#pragma unroll
                    for (int a = 0; a < NZ; ++a)
#pragma unroll
                        for (int b = 0; b < NZ; ++b) {
                            double s;
                            if (b + Z0 == 0) {
                                s = KM[a][b];
                            } else {
                                const int k = b + Z0 - 1;
                                s = 0.0;
#pragma unroll
                                for (int j = 0; j < G; ++j) s += KM[a][1 + j - Z0] * K[k][j];
                            }
                            P[((i * BS + jj) * NZ + a) * NZ + b] = scale * s;
                        }
                }
        }
        __syncthreads();
        // phase 2: thread = (cell, a, b)
        for (int t = threadIdx.x; t < ncell * nd * nd; t += blockDim.x) {
            const int c = t / (nd * nd), ab = t - c * nd * nd, a = ab / nd, b = ab - a * nd;
            double acc[BS][BS];
#pragma unroll
            for (int i = 0; i < BS; ++i)
#pragma unroll
                for (int j = 0; j < BS; ++j) acc[i][j] = 0.0;
            for (int q = 0; q < nq; ++q) {
                double za[NZ], zb[NZ];
                if constexpr (Z0 == 0) {
                    za[0] = tab[q * L.sphi + a];
                    zb[0] = tab[q * L.sphi + b];
                }
                const double* dp = tab + L.o_dphi + q * L.sdphi;
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    za[1 + k - Z0] = dp[a * G + k];
                    zb[1 + k - Z0] = dp[b * G + k];
                }
                const double* P = Ms + (c * nq + q) * PS;
#pragma unroll
                for (int z1 = 0; z1 < NZ; ++z1)
#pragma unroll
                    for (int z2 = 0; z2 < NZ; ++z2) {
                        const double zz = za[z1] * zb[z2];
#pragma unroll
                        for (int i = 0; i < BS; ++i)
#pragma unroll
                            for (int j = 0; j < BS; ++j) acc[i][j] += zz * P[((i * BS + j) * NZ + z1) * NZ + z2];
                    }
            }
            const int64_t cell = c0 + c;
            if (ae) {
                double* dst = ae + ((cell - c_begin) * ndb + (int64_t)a * BS) * ndb + b * BS;
#pragma unroll
                for (int i = 0; i < BS; ++i)
#pragma unroll
                    for (int j = 0; j < BS; ++j) dst[(int64_t)i * ndb + j] = acc[i][j];
            } else {
                const int64_t na = m.dofmap[cell * nd + a];
                const int64_t blk = (int64_t)pos[(cell * nd + a) * nd + b] * BS;
#pragma unroll
                for (int i = 0; i < BS; ++i)
#pragma unroll
                    for (int j = 0; j < BS; ++j) unsafeAtomicAdd(values + row_ptr[na * BS + i] + blk + j, acc[i][j]);
            }
        }
        __syncthreads();    // X and Ms are rewritten by the next group
    }
}

__global__ __launch_bounds__(DXO_AS_BLOCK) void dirichlet_mark(const int32_t* __restrict__ dofs, int64_t n_dofs, int64_t n_rows,
                                                               uint8_t* __restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_dofs; k += stride) {
        const int32_t d = dofs[k];
        if (d >= 0 && d < n_rows) mask[d] = 1;      // out-of-range entries are ignored
    }
}

// one owner per row: a constrained row becomes diagonal * e_r; the other rows lose their constrained columns
__global__ __launch_bounds__(DXO_AS_BLOCK) void dirichlet_rows(int64_t n_rows, const int64_t* __restrict__ row_ptr,
                                                               const int32_t* __restrict__ col, const uint8_t* __restrict__ mask,
                                                               double diagonal, double* __restrict__ values) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) {
        const int64_t e0 = row_ptr[r], e1 = row_ptr[r + 1];
        if (mask[r]) {
            for (int64_t e = e0; e < e1; ++e) values[e] = col[e] == r ? diagonal : 0.0;
        } else {
            for (int64_t e = e0; e < e1; ++e)
                if (mask[col[e]]) values[e] = 0.0;
        }
    }
}

// ---- host side
struct AssembleOps {
    size_t (*lds_bytes)(const dxo_mesh*, int) = nullptr;
    void (*launch)(const dxo_mesh*, const dxo_csr*, int, int, size_t, const double*, int64_t, int64_t, double*, double*, hipStream_t) = nullptr;
};

template <int G, int BS, int TEST, int TRIAL>
struct Assemble {
    static size_t lds_bytes(const dxo_mesh* mesh, int cpb) {
        const OperandDev& d = mesh->dev;
        const int sx = op_odd(d.ngeom * G);
        return (size_t)(d.table_doubles + ((cpb * sx + 1) & ~1) + cpb * d.nq * AsShape<G, BS, TEST, TRIAL>::PS) * sizeof(double);
    }
    static void launch(const dxo_mesh* mesh, const dxo_csr* csr, int cpb, int blocks, size_t shm, const double* C, int64_t c0, int64_t c1,
                       double* ae, double* values, hipStream_t s) {
        hipLaunchKernelGGL((assemble_elem<G, BS, TEST, TRIAL>), dim3(blocks), dim3(DXO_AS_BLOCK), shm, s, mesh->dev, mesh->d_wq, C, c0, c1,
                           cpb, ae, csr->d_row_ptr, csr->d_pos, values);
    }
};

int grid_blocks(const dxo_ctx* ctx, int64_t work, int per_block) { return capped_grid(ctx, work, per_block, DXO_AS_BLOCKS_PER_CU); }

void csr_free(dxo_csr* c) {
    free_all({c->d_row_ptr, c->d_col, c->d_inc_ptr, c->d_inc, c->d_pos, c->d_mask, c->d_mirror, c->d_ae});
    delete c;
}

int csr_build(dxo_ctx* ctx, dxo_csr* c, const dxo_mesh* mesh) {
    const int64_t nc = mesh->num_cells, nd = mesh->dev.ndofs, nn = mesh->num_field_nodes, bs = c->bs;
    const std::vector<int32_t>& dm = mesh->h_dofmap;
    if ((int64_t)dm.size() != nc * nd) return dxo_fail(ctx, DXO_E_DIM, "dxo_csr_create: the mesh keeps no host dofmap");
    // incidences, ascending (cell, a) per node
    std::vector<int64_t> inc_ptr;
    std::vector<uint32_t> inc;
    if (!transpose_incidence(nc * nd, nn, [&](int64_t e) { return dm[(size_t)e]; }, [](int64_t e) { return e; }, inc_ptr, inc))
        return dxo_fail(ctx, DXO_E_SIZE, "dxo_csr_create: dofmap entry out of range");
    // sorted neighbour nodes per node
    std::vector<int64_t> nb_ptr((size_t)nn + 1, 0);
    std::vector<int32_t> nb;
    nb.reserve((size_t)(nc * nd * 4));
    std::vector<int32_t> tmp;
    for (int64_t n = 0; n < nn; ++n) {
        tmp.clear();
        for (int64_t e = inc_ptr[(size_t)n]; e < inc_ptr[(size_t)n + 1]; ++e) {
            const int64_t cell = inc[(size_t)e] / nd;
            tmp.insert(tmp.end(), dm.begin() + cell * nd, dm.begin() + (cell + 1) * nd);
        }
        tmp.push_back((int32_t)n);      // the diagonal, also for a node in no cell
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        if (tmp.size() >= 65536) return dxo_fail(ctx, DXO_E_SIZE, "dxo_csr_create: a node has 65536 or more neighbours");
        nb.insert(nb.end(), tmp.begin(), tmp.end());
        nb_ptr[(size_t)n + 1] = (int64_t)nb.size();
    }
    // rows: node-major, component-minor; every row of node n is bs * |nb(n)| long
    c->n_rows = nn * bs;
    std::vector<int64_t> row_ptr((size_t)c->n_rows + 1, 0);
    for (int64_t n = 0; n < nn; ++n)
        for (int64_t i = 0; i < bs; ++i)
            row_ptr[(size_t)(n * bs + i) + 1] = row_ptr[(size_t)(n * bs + i)] + bs * (nb_ptr[(size_t)n + 1] - nb_ptr[(size_t)n]);
    c->nnz = row_ptr.back();
    std::vector<int32_t> col((size_t)c->nnz);
    for (int64_t n = 0; n < nn; ++n)
        for (int64_t i = 0; i < bs; ++i) {
            int64_t w = row_ptr[(size_t)(n * bs + i)];
            for (int64_t k = nb_ptr[(size_t)n]; k < nb_ptr[(size_t)n + 1]; ++k)
                for (int64_t j = 0; j < bs; ++j) col[(size_t)w++] = (int32_t)(nb[(size_t)k] * bs + j);
        }
    // column block of b's node in the rows of a's node
    std::vector<uint16_t> pos((size_t)(nc * nd * nd));
    for (int64_t cell = 0; cell < nc; ++cell)
        for (int64_t a = 0; a < nd; ++a) {
            const int32_t na = dm[(size_t)(cell * nd + a)];
            const int32_t* lo = nb.data() + nb_ptr[(size_t)na];
            const int32_t* hi = nb.data() + nb_ptr[(size_t)na + 1];
            for (int64_t b = 0; b < nd; ++b)
                pos[(size_t)((cell * nd + a) * nd + b)] = (uint16_t)(std::lower_bound(lo, hi, dm[(size_t)(cell * nd + b)]) - lo);
        }
    // + 16 bytes: kernels read whole vectors past the end
    int rc = to_device(ctx, &c->d_row_ptr, row_ptr, 16);
    if (rc == DXO_OK) rc = to_device(ctx, &c->d_col, col, 16);
    if (rc == DXO_OK) rc = to_device(ctx, &c->d_inc_ptr, inc_ptr, 16);
    if (rc == DXO_OK) rc = to_device(ctx, &c->d_inc, inc, 16);
    if (rc == DXO_OK) rc = to_device(ctx, &c->d_pos, pos, 16);
    if (rc != DXO_OK) return rc;
    DXO_HIP(ctx, hipMalloc((void**)&c->d_mask, (size_t)c->n_rows + 16));
    return DXO_OK;
}

int assemble_impl(dxo_ctx* ctx, dxo_mesh* mesh, dxo_csr* csr, int test, int trial, int bs, const double* C, double* values) {
    const char* who = "dxo_bilinear_assemble";
    if (!mesh || !csr || !C || !values) return dxo_fail(ctx, DXO_E_NULL, "dxo_bilinear_assemble: NULL argument");
    AssembleOps ops;
    int rc = bilinear_pair_check(ctx, who, mesh, test, trial, bs, ops, [](auto G, auto BS, auto T, auto R) {
        return AssembleOps{&Assemble<G, BS, T, R>::lds_bytes, &Assemble<G, BS, T, R>::launch};
    });
    if (rc != DXO_OK) return rc;
    if (csr->mesh != mesh || csr->bs != bs) {
        char msg[320];
        snprintf(msg, sizeof msg, "%s: the pattern was made for another mesh or block size (pattern bs %d, call bs %d)", who, csr->bs, bs);
        return dxo_fail(ctx, DXO_E_DIM, msg);
    }
    if (((uintptr_t)C & 15u) != 0) return fail_who(ctx, DXO_E_ALIGN, who, "C must be 16-byte aligned");
    const int nd = mesh->dev.ndofs;
    int cpb = DXO_AS_BLOCK / (nd * nd);
    if (cpb < 1) cpb = 1;
    if (cpb > 64) cpb = 64;
    while (cpb > 1 && ops.lds_bytes(mesh, cpb) > 64 * 1024) cpb /= 2;
    const size_t shm = ops.lds_bytes(mesh, cpb);
    if (shm > 64 * 1024) return fail_who(ctx, DXO_E_SIZE, who, "element too large for the LDS budget");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t nc = mesh->num_cells;
    const size_t cell_bytes = (size_t)nd * bs * nd * bs * sizeof(double);
    auto begin = [&]() -> int {
        const int rc = dxo_device_begin(ctx, s);
        if (rc != DXO_OK) return rc;
        if (ctx->consumer_overwrite) DXO_HIP(ctx, hipMemsetAsync(values, 0, (size_t)csr->nnz * sizeof(double), s));
        return DXO_OK;
    };
    if (ctx->adjoint_atomics || nc == 0) {
        rc = begin();
        if (rc == DXO_OK && nc > 0) ops.launch(mesh, csr, cpb, grid_blocks(ctx, (nc + cpb - 1) / cpb, 1), shm, C, 0, nc, nullptr, values, s);
    } else {
        const int rblocks = grid_blocks(ctx, csr->n_rows, DXO_AS_BLOCK);
        const CellRows rows{csr->n_nodes, csr->d_inc_ptr, csr->d_inc};
        rc = assemble_two_pass(
            ctx, nc, cell_bytes, &csr->d_ae, &csr->ae_cap, begin,
            [&](int64_t c0, int64_t c1) {
                ops.launch(mesh, csr, cpb, grid_blocks(ctx, (c1 - c0 + cpb - 1) / cpb, 1), shm, C, c0, c1, csr->d_ae, values, s);
            },
            [&](int64_t c0, int64_t c1) {
                with_node_bs(bs, [&](auto BS) {
                    hipLaunchKernelGGL((assemble_rows<BS, DXO_AS_BLOCK, CellRows>), dim3(rblocks), dim3(DXO_AS_BLOCK), 0, s, rows, nd, csr->d_row_ptr,
                                       csr->d_pos, csr->d_ae, c0, c1, values);
                });
            });
    }
    return rc != DXO_OK ? rc : dxo_device_end(ctx, s);
}

}  // namespace

extern "C" int dxo_csr_create(dxo_ctx* ctx, dxo_mesh* mesh, int bs, dxo_csr** out) {
    if (!ctx || !mesh || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    if (bs != 1 && bs != mesh->gdim) return dxo_fail(ctx, DXO_E_DIM, "dxo_csr_create: bs must be 1 or gdim");
    if (mesh->num_field_nodes * bs >= ((int64_t)1 << 31)) return dxo_fail(ctx, DXO_E_SIZE, "dxo_csr_create: 2^31 or more dofs (int32 columns)");
    if (mesh->num_cells * mesh->dev.ndofs >= ((int64_t)1 << 32)) return dxo_fail(ctx, DXO_E_SIZE, "dxo_csr_create: 2^32 or more (cell, node) entries");
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    const auto t0 = std::chrono::steady_clock::now();
    dxo_csr* c = new dxo_csr;
    c->mesh = mesh;
    c->bs = bs;
    c->nd = mesh->dev.ndofs;
    c->n_nodes = mesh->num_field_nodes;
    c->n_cells = mesh->num_cells;
    const int rc = csr_build(ctx, c, mesh);
    if (rc != DXO_OK) {
        csr_free(c);
        return rc;
    }
    c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = c;
    return DXO_OK;
}

extern "C" int dxo_csr_destroy(dxo_ctx* ctx, dxo_csr* csr) {
    if (!csr) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (ctx) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();       // the scratch may still be read by a queued launch
    csr_free(csr);
    return DXO_OK;
}

extern "C" int dxo_csr_info(dxo_ctx* ctx, const dxo_csr* csr, int64_t* n_rows, int64_t* nnz, const int64_t** row_ptr, const int32_t** col,
                            double* build_ms) {
    if (!csr) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (n_rows) *n_rows = csr->n_rows;
    if (nnz) *nnz = csr->nnz;
    if (row_ptr) *row_ptr = csr->d_row_ptr;
    if (col) *col = csr->d_col;
    if (build_ms) *build_ms = csr->build_ms;
    return DXO_OK;
}

extern "C" int dxo_bilinear_assemble(dxo_ctx* ctx, dxo_mesh* mesh, dxo_csr* csr, int test_kind, int trial_kind, int bs, const double* C,
                                     double* values) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    return assemble_impl(ctx, mesh, csr, test_kind, trial_kind, bs, C, values);
}

extern "C" int dxo_csr_dirichlet(dxo_ctx* ctx, dxo_csr* csr, const int32_t* dofs, int64_t n_dofs, double diagonal, double* values) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!csr || !values || (n_dofs > 0 && !dofs)) return dxo_fail(ctx, DXO_E_NULL, "dxo_csr_dirichlet: NULL argument");
    if (n_dofs < 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_csr_dirichlet: n_dofs < 0");
    if (!csr->mesh) return dxo_fail(ctx, DXO_E_DIM, "dxo_csr_dirichlet: a pattern without a mesh (a multigrid level) keeps no mask");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    if (n_dofs > 0 && csr->n_rows > 0) {
        DXO_HIP(ctx, hipMemsetAsync(csr->d_mask, 0, (size_t)csr->n_rows, s));
        hipLaunchKernelGGL(dirichlet_mark, dim3(grid_blocks(ctx, n_dofs, DXO_AS_BLOCK)), dim3(DXO_AS_BLOCK), 0, s, dofs, n_dofs, csr->n_rows,
                           csr->d_mask);
        hipLaunchKernelGGL(dirichlet_rows, dim3(grid_blocks(ctx, csr->n_rows, DXO_AS_BLOCK)), dim3(DXO_AS_BLOCK), 0, s, csr->n_rows,
                           csr->d_row_ptr, csr->d_col, csr->d_mask, diagonal, values);
    }
    return dxo_device_end(ctx, s);
}
