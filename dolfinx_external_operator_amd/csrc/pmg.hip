// pmg.hip — dxo_pmg_*: a two-level p-multigrid cycle whose fine level is an OPERATOR (a matrix or a callback), not a matrix.
//
// The fine level is smoothed by the Chebyshev polynomial in Dinv A on [lower rho, rho], Dinv the inverse DIAGONAL the caller hands in
// (1 on constrained dofs) and rho the power estimate of dxo_amg_set_smoother made on the operator. The residual goes to the degree-1
// space on the same cells by the nodal interpolation P = W (x) I_bs of dxo_amg_create_transfer (stored as the diagonals of its blocks,
// p_diag [block][bs], constrained dofs removed on both sides), any preconditioner of a matrix of that space corrects it, and the same
// polynomial runs again from the corrected iterate. Nothing here needs an entry of the fine matrix.
//
// Symbolic part (dxo_pmg_create, host C++): the checks of the transfer, p_diag, the transposed incidence of P (coarse node -> its
// blocks, fine nodes ascending, so that the restriction is a gather) and the constrained dofs of the coarse space. All device memory
// of setup and apply is allocated there.
//
// Kernels, all bandwidth-bound, grid-stride with 64-bit indices, every vector touched once:
//   pmg_cheby<FIRST>   FIRST: d = c2 dinv r, x = d (no operator product behind it, nothing read but r and dinv);
//                      otherwise d = c1 d + c2 dinv (r - t), out = x + d with t = A x. Two entries per thread as one 16-byte access
//                      where the pointers allow, the pair (c1, c2) read from device memory.
//   pmg_restrict       r_c[v][c] = sum over the blocks (i, v), ascending i, of p_diag (r_i[c] - t_i[c]) (t NULL: of p_diag r_i[c]):
//                      the residual is never stored.
//   pmg_prolong<ADD>   x_i[c] (+)= sum over the blocks of row i, ascending v, of p_diag e_v[c].
//   pmg_power_init / pmg_scale / pmg_dinv_norm / pmg_power_norm   the power iteration w <- Dinv A (w / |w|): the start vector of the
//                      multigrid, |w|^2 as per-workgroup partials on a grid that depends on n alone (a thread adds its entries in
//                      ascending order, then the xor-butterfly of the wave, then the waves in ascending order), the partials added
//                      by one workgroup in the same manner. After the last step that workgroup leaves rho = safety |w| and the
//                      Chebyshev pairs on the device: no host read anywhere.
#include "dxo_common.h"
#include "krylov_internal.h"
#include "pmg_symbolic.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace {

constexpr int PMG_BLOCK = 256;
constexpr int PMG_MAX_PARTS = 1024;      // workgroups of a reduction: a function of n alone, never of the device
constexpr int PMG_MAX_DEGREE = 8;

}  // namespace

struct dxo_pmg {
    int device = 0;
    int bs = 1;
    int64_t n_nodes = 0, n = 0;            // fine nodes and rows
    int64_t n_coarse = 0, nc = 0;          // coarse nodes and rows
    int64_t p_blocks = 0;
    // the transfer, on the device
    int64_t* p_ptr = nullptr;              // [n_nodes + 1]
    int32_t* p_col = nullptr;              // [p_blocks] coarse node
    double* p_diag = nullptr;              // [p_blocks][bs]
    int64_t* pt_ptr = nullptr;             // [n_coarse + 1] blocks of a coarse node ...
    int64_t* pt_blk = nullptr;             // [p_blocks] ... as positions in p_col / p_diag, fine nodes ascending
    int32_t* pt_row = nullptr;             // [p_blocks] the fine node of block pt_blk[e]
    int32_t* c_bc = nullptr;               // [n_c_bc] constrained dofs of the coarse space, ascending
    int64_t n_c_bc = 0;
    // vectors
    double *x = nullptr, *d = nullptr, *t = nullptr, *w = nullptr;      // [n]; w: the power iteration
    double *rc = nullptr, *ec = nullptr;                                  // [nc]
    double* part = nullptr;                // [PMG_MAX_PARTS]
    double* scal = nullptr;                // [0] 1 / |w|, [1] |w|, [2] rho, [4 ..] the pairs (c1, c2) of the steps
    // the smoother
    int degree = 2, rho_iters = 10;
    double lower = 0.1, safety = 1.1;
    int set_degree = 2;                    // what the last setup ran with (the pairs on the device)
    bool ready = false;
    // what the last setup was given
    dxo_krylov_op fine = {};
    const double* dinv = nullptr;
    dxo_krylov_pc coarse = {};
    dxo_krylov_callback coarse_cb = {};
    double* rho() const { return scal + 2; }
    double* pairs() const { return scal + 4; }
};

namespace {

// ---- device code
// the sum of s over the workgroup, on every thread: the xor-butterfly of a wave, then the waves in ascending order
__device__ __forceinline__ double pmg_block_sum(double s, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = lds[0];
#pragma unroll
    for (int k = 1; k < PMG_BLOCK / 64; ++k) t += lds[k];
    return t;
}

// w[i] = 0.5 + ((uint32)(i * 2654435761) >> 8) * 2^-24 (exact in fp64) and the workgroups' partials of |w|^2
__global__ __launch_bounds__(PMG_BLOCK) void pmg_power_init(int64_t n, double* __restrict__ w, double* __restrict__ part) {
    __shared__ double lds[PMG_BLOCK / 64];
    const int64_t stride = (int64_t)gridDim.x * PMG_BLOCK;
    double q = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * PMG_BLOCK + threadIdx.x; i < n; i += stride) {
        const double v = 0.5 + (double)(((uint32_t)i * 2654435761u) >> 8) * 0x1p-24;
        w[i] = v;
        q = fma(v, v, q);
    }
    q = pmg_block_sum(q, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// v = scal[0] w: the normalised vector the operator is given
__global__ __launch_bounds__(PMG_BLOCK) void pmg_scale(int64_t n, const double* __restrict__ scal, const double* __restrict__ w,
                                                       double* __restrict__ v) {
    const int64_t stride = (int64_t)gridDim.x * PMG_BLOCK;
    const double s = scal[0];
    for (int64_t i = (int64_t)blockIdx.x * PMG_BLOCK + threadIdx.x; i < n; i += stride) v[i] = s * w[i];
}

// w = dinv a (a = A v) and the workgroups' partials of |w|^2
__global__ __launch_bounds__(PMG_BLOCK) void pmg_dinv_norm(int64_t n, const double* __restrict__ dinv, const double* __restrict__ a,
                                                           double* __restrict__ w, double* __restrict__ part) {
    __shared__ double lds[PMG_BLOCK / 64];
    const int64_t stride = (int64_t)gridDim.x * PMG_BLOCK;
    double q = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * PMG_BLOCK + threadIdx.x; i < n; i += stride) {
        const double v = dinv[i] * a[i];
        w[i] = v;
        q = fma(v, v, q);
    }
    q = pmg_block_sum(q, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// the pairs (c1, c2) of the steps d = c1 d + c2 Dinv (r - A x), x += d of the Chebyshev polynomial of `degree` on [lower rho, rho]
// (the recurrence documented at dxo_amg_set_smoother); rho not > 0: no relaxation
__device__ __forceinline__ void pmg_cheby_table(double rho, double lower, int degree, double* __restrict__ c) {
    if (!(rho > 0.0)) {
        for (int k = 0; k < 2 * degree; ++k) c[k] = 0.0;
        return;
    }
    const double a = lower * rho, theta = 0.5 * (a + rho), delta = 0.5 * (rho - a), sigma = theta / delta;
    double r0 = 1.0 / sigma;
    c[0] = 0.0;
    c[1] = 1.0 / theta;
    for (int k = 1; k < degree; ++k) {
        const double r1 = 1.0 / (2.0 * sigma - r0);
        c[2 * k] = r1 * r0;
        c[2 * k + 1] = 2.0 * r1 / delta;
        r0 = r1;
    }
}

// one workgroup: |w| from the nb partials (a thread's partials in ascending order, then pmg_block_sum); scal = (1 / |w|, |w|) for the
// next step. After the last step rho = safety |w| and the pairs
__global__ __launch_bounds__(PMG_BLOCK) void pmg_power_norm(const double* __restrict__ part, int nb, int last, double safety, double lower,
                                                            int degree, double* __restrict__ scal) {
    __shared__ double lds[PMG_BLOCK / 64];
    double q = 0.0;
    for (int i = threadIdx.x; i < nb; i += PMG_BLOCK) q += part[i];
    q = pmg_block_sum(q, lds);
    if (threadIdx.x != 0) return;
    const double lam = sqrt(q);
    scal[0] = lam > 0.0 ? 1.0 / lam : 0.0;
    scal[1] = lam;
    if (last) {
        const double r = safety * lam;
        scal[2] = r;
        pmg_cheby_table(r, lower, degree, scal + 4);
    }
}

// one entry of a step of the polynomial
__device__ __forceinline__ double pmg_step(double c1, double c2, double dinv, double r, double t, double d) { return fma(c1, d, c2 * (dinv * (r - t))); }

// FIRST: d = c2 dinv r, out = d. Otherwise d = c1 d + c2 dinv (r - t), out = x + d. `wide`: every pointer is 16-byte aligned, so a
// thread takes the entries 2 j, 2 j + 1 as one double2 (the last entry of an odd n alone). r may be out, x may be out: no __restrict__
template <bool FIRST>
__global__ __launch_bounds__(PMG_BLOCK) void pmg_cheby(int64_t n, int wide, const double* __restrict__ pair, const double* __restrict__ dinv,
                                                       const double* r, const double* t, double* d, const double* x, double* out) {
    const int64_t stride = (int64_t)gridDim.x * PMG_BLOCK;
    const int64_t first = (int64_t)blockIdx.x * PMG_BLOCK + threadIdx.x;
    const double c1 = pair[0], c2 = pair[1];
    if (wide) {
        const int64_t n2 = n >> 1;
        for (int64_t j = first; j < n2; j += stride) {
            const double2 di = reinterpret_cast<const double2*>(dinv)[j], rr = reinterpret_cast<const double2*>(r)[j];
            double2 dd;
            if constexpr (FIRST) {
                dd.x = c2 * (di.x * rr.x);
                dd.y = c2 * (di.y * rr.y);
                reinterpret_cast<double2*>(d)[j] = dd;
                reinterpret_cast<double2*>(out)[j] = dd;
            } else {
                const double2 tt = reinterpret_cast<const double2*>(t)[j], d0 = reinterpret_cast<const double2*>(d)[j],
                              xx = reinterpret_cast<const double2*>(x)[j];
                dd.x = pmg_step(c1, c2, di.x, rr.x, tt.x, d0.x);
                dd.y = pmg_step(c1, c2, di.y, rr.y, tt.y, d0.y);
                reinterpret_cast<double2*>(d)[j] = dd;
                double2 o;
                o.x = xx.x + dd.x;
                o.y = xx.y + dd.y;
                reinterpret_cast<double2*>(out)[j] = o;
            }
        }
        if ((n & 1) && first == 0) {
            const int64_t i = n - 1;
            if constexpr (FIRST) {
                const double dd = c2 * (dinv[i] * r[i]);
                d[i] = dd;
                out[i] = dd;
            } else {
                const double dd = pmg_step(c1, c2, dinv[i], r[i], t[i], d[i]);
                d[i] = dd;
                out[i] = x[i] + dd;
            }
        }
        return;
    }
    for (int64_t i = first; i < n; i += stride) {
        if constexpr (FIRST) {
            const double dd = c2 * (dinv[i] * r[i]);
            d[i] = dd;
            out[i] = dd;
        } else {
            const double dd = pmg_step(c1, c2, dinv[i], r[i], t[i], d[i]);
            d[i] = dd;
            out[i] = x[i] + dd;
        }
    }
}

// r_c[v][c] = sum over the blocks (i, v) of P, ascending i, of p_diag[block][c] (r_i[c] - t_i[c]); t NULL: of p_diag[block][c] r_i[c].
// One thread per coarse dof: consecutive lanes read consecutive entries of p_diag, r and t
template <int BS, bool RESIDUAL>
__global__ __launch_bounds__(PMG_BLOCK) void pmg_restrict(int64_t nc, const int64_t* __restrict__ pt_ptr, const int64_t* __restrict__ pt_blk,
                                                          const int32_t* __restrict__ pt_row, const double* __restrict__ p_diag,
                                                          const double* __restrict__ r, const double* __restrict__ t, double* __restrict__ rc) {
    const int64_t stride = (int64_t)gridDim.x * PMG_BLOCK;
    for (int64_t g = (int64_t)blockIdx.x * PMG_BLOCK + threadIdx.x; g < nc; g += stride) {
        const int64_t v = g / BS;
        const int c = (int)(g % BS);
        double acc = 0.0;
        for (int64_t e = pt_ptr[v]; e < pt_ptr[v + 1]; ++e) {
            const int64_t pb = pt_blk[e], i = (int64_t)pt_row[e] * BS + c;
            const double res = RESIDUAL ? r[i] - t[i] : r[i];
            acc = fma(p_diag[pb * BS + c], res, acc);
        }
        rc[g] = acc;
    }
}

// x_i[c] = (ADD ? x_i[c] : 0) + sum over the blocks of row i, ascending coarse node, of p_diag[block][c] e_v[c]
template <int BS, bool ADD>
__global__ __launch_bounds__(PMG_BLOCK) void pmg_prolong(int64_t n, const int64_t* __restrict__ p_ptr, const int32_t* __restrict__ p_col,
                                                         const double* __restrict__ p_diag, const double* __restrict__ ec, double* __restrict__ x) {
    const int64_t stride = (int64_t)gridDim.x * PMG_BLOCK;
    for (int64_t g = (int64_t)blockIdx.x * PMG_BLOCK + threadIdx.x; g < n; g += stride) {
        const int64_t i = g / BS;
        const int c = (int)(g % BS);
        double acc = 0.0;
        for (int64_t e = p_ptr[i]; e < p_ptr[i + 1]; ++e) acc = fma(p_diag[e * BS + c], ec[(int64_t)p_col[e] * BS + c], acc);
        x[g] = ADD ? x[g] + acc : acc;
    }
}

// ---- host side
// The objects dxo_pmg_create has made and dxo_pmg_destroy has not yet freed. dxo_krylov_pc::inv is an untyped pointer: before
// DXO_PC_PMG existed, 5 was an unknown kind (DXO_E_OPTION) whatever inv carried, so a pointer that is not one of these objects is
// refused with that code and never read.
std::mutex pmg_live_mu;
std::set<const dxo_pmg*> pmg_live;
bool pmg_is_live(const dxo_pmg* p) {
    std::lock_guard<std::mutex> g(pmg_live_mu);
    return pmg_live.count(p) != 0;
}

bool pmg_misaligned(const void* p) { return ((uintptr_t)p & 7u) != 0; }
bool pmg_wide(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (p && ((uintptr_t)p & 15u) != 0) return false;
    return true;
}

// the grid of the elementwise and transfer kernels: one thread per `per` entries up to a cap that covers the device a few times
// over (option "pmg_grid_blocks": the cap; every entry is computed by one thread on its own, so the results do not depend on it)
dim3 pmg_grid(const dxo_ctx* ctx, int64_t n, int64_t per = 1) {
    const int64_t want = (n / per + PMG_BLOCK) / PMG_BLOCK;
    const int64_t cap = ctx->pmg_grid_blocks > 0 ? ctx->pmg_grid_blocks : (int64_t)std::max(1, ctx->compute_units) * 16;
    return dim3((unsigned)std::max<int64_t>(1, std::min(want, cap)));
}
// the grid of a reduction: a function of n alone
int pmg_parts(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(PMG_MAX_PARTS, (n + PMG_BLOCK - 1) / PMG_BLOCK)); }

const auto pmg_no_shape = [](int v) {
    fprintf(stderr, "pmg.hip: no kernel instantiation for block size %d\n", v);
    std::abort();
};

void pmg_free(dxo_pmg* p) {
    for (void* q : {(void*)p->p_ptr, (void*)p->p_col, (void*)p->p_diag, (void*)p->pt_ptr, (void*)p->pt_blk, (void*)p->pt_row, (void*)p->c_bc, (void*)p->x,
                    (void*)p->d, (void*)p->t, (void*)p->w, (void*)p->rc, (void*)p->ec, (void*)p->part, (void*)p->scal})
        if (q) (void)hipFree(q);
    delete p;
}

template <class T>
hipError_t pmg_upload(T** dev, const std::vector<T>& host) {
    const size_t bytes = std::max<size_t>(host.size(), 1) * sizeof(T);
    hipError_t e = hipMalloc((void**)dev, bytes);
    if (e == hipSuccess && !host.empty()) e = hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

hipError_t pmg_zeros(double** dev, int64_t n) {
    const size_t bytes = (size_t)std::max<int64_t>(n, 1) * sizeof(double);
    hipError_t e = hipMalloc((void**)dev, bytes);
    if (e == hipSuccess) e = hipMemset(*dev, 0, bytes);
    return e;
}

struct PmgRun {
    dxo_ctx* ctx;
    dxo_pmg* p;
    hipStream_t s;
    // out = A v
    int op(const double* v, double* out) const {
        const dxo_krylov_op& A = p->fine;
        if (A.csr) return dxo_kr_spmv_launch(ctx, A.csr, A.values, v, out, s);
        const int rc = A.apply(A.user, v, out);
        if (rc != DXO_OK) {
            char msg[128];
            snprintf(msg, sizeof msg, "dxo_pmg: the operator callback returned %d", rc);
            return dxo_fail(ctx, rc < 0 ? rc : DXO_E_OPTION, msg);
        }
        return DXO_OK;
    }
    // e_c = M_c r_c
    int coarse(const double* rc, double* ec) const {
        const dxo_krylov_pc& M = p->coarse;
        if (M.kind == DXO_PC_AMG) {
            dxo_amg_cycle(ctx, (dxo_amg*)M.inv, rc, ec, s);
            return DXO_OK;
        }
        if (M.kind == DXO_PC_CALLBACK) {
            const int r = p->coarse_cb.apply(p->coarse_cb.user, rc, ec);
            if (r != DXO_OK) {
                char msg[128];
                snprintf(msg, sizeof msg, "dxo_pmg: the coarse preconditioner callback returned %d", r);
                return dxo_fail(ctx, r < 0 ? r : DXO_E_OPTION, msg);
            }
            return DXO_OK;
        }
        return dxo_kr_bj_apply_launch(ctx, "dxo_pmg", M.kind == DXO_PC_JACOBI ? 1 : M.bs, p->nc, M.inv, rc, ec, s);
    }
    void cheby_first(const double* pair, const double* r, double* out) const {
        const int wide = pmg_wide({p->dinv, r, p->d, out}) ? 1 : 0;
        hipLaunchKernelGGL(pmg_cheby<true>, pmg_grid(ctx, p->n, wide ? 2 : 1), dim3(PMG_BLOCK), 0, s, p->n, wide, pair, p->dinv, r, (const double*)nullptr,
                           p->d, (const double*)nullptr, out);
    }
    void cheby(const double* pair, const double* r, const double* x, double* out) const {
        const int wide = pmg_wide({p->dinv, r, p->t, p->d, x, out}) ? 1 : 0;
        hipLaunchKernelGGL(pmg_cheby<false>, pmg_grid(ctx, p->n, wide ? 2 : 1), dim3(PMG_BLOCK), 0, s, p->n, wide, pair, p->dinv, r, (const double*)p->t,
                           p->d, x, out);
    }
    // r_c = P^T (r - t), t NULL: P^T r
    void restrict_(const double* r, const double* t, double* rc) const {
        if (p->nc == 0) return;
        with_int<1, 2, 3>(p->bs, [&](auto BS) {
            if (t)
                hipLaunchKernelGGL((pmg_restrict<BS, true>), pmg_grid(ctx, p->nc), dim3(PMG_BLOCK), 0, s, p->nc, p->pt_ptr, p->pt_blk, p->pt_row, p->p_diag, r,
                                   t, rc);
            else
                hipLaunchKernelGGL((pmg_restrict<BS, false>), pmg_grid(ctx, p->nc), dim3(PMG_BLOCK), 0, s, p->nc, p->pt_ptr, p->pt_blk, p->pt_row, p->p_diag,
                                   r, (const double*)nullptr, rc);
        }, pmg_no_shape);
    }
    void prolong(const double* ec, double* x, bool add) const {
        if (p->n == 0) return;
        with_int<1, 2, 3>(p->bs, [&](auto BS) {
            if (add) hipLaunchKernelGGL((pmg_prolong<BS, true>), pmg_grid(ctx, p->n), dim3(PMG_BLOCK), 0, s, p->n, p->p_ptr, p->p_col, p->p_diag, ec, x);
            else hipLaunchKernelGGL((pmg_prolong<BS, false>), pmg_grid(ctx, p->n), dim3(PMG_BLOCK), 0, s, p->n, p->p_ptr, p->p_col, p->p_diag, ec, x);
        }, pmg_no_shape);
    }
};

int pmg_check_vectors(dxo_ctx* ctx, const char* who, const dxo_pmg* pmg, const void* a, const void* b) {
    if (!pmg || !a || !b) return fail_who(ctx, DXO_E_NULL, who, "NULL argument");
    if (pmg_misaligned(a) || pmg_misaligned(b)) return fail_who(ctx, DXO_E_ALIGN, who, "arrays must be 8-byte aligned");
    return DXO_OK;
}

}  // namespace

// ---- shared with krylov.hip
int dxo_pmg_pc_check(dxo_ctx* ctx, const char* who, const dxo_pmg* pmg, const dxo_csr* op_csr, int64_t n) {
    char msg[256];
    if (!pmg) return fail_who(ctx, DXO_E_NULL, who, "the preconditioner carries no dxo_pmg");
    if (!pmg_is_live(pmg)) return fail_who(ctx, DXO_E_OPTION, who, "kind DXO_PC_PMG, but inv is not an object of dxo_pmg_create (or it was destroyed)");
    if (op_csr && op_csr->bs != pmg->bs) {
        snprintf(msg, sizeof msg, "p-multigrid of bs %d on a pattern of bs %d", pmg->bs, op_csr->bs);
        return fail_who(ctx, DXO_E_DIM, who, msg);
    }
    if (n != pmg->n) {
        snprintf(msg, sizeof msg, "the p-multigrid covers %lld rows, the operator has %lld", (long long)pmg->n, (long long)n);
        return fail_who(ctx, DXO_E_SIZE, who, msg);
    }
    if (!pmg->ready) return fail_who(ctx, DXO_E_OPTION, who, "dxo_pmg_setup has not run (or failed, or dxo_pmg_set_smoother came after it)");
    return DXO_OK;
}

// z = M r on the stream: 2 degree operator products, one coarse preconditioner call; r may be z
int dxo_pmg_cycle(dxo_ctx* ctx, dxo_pmg* p, const double* r, double* z, hipStream_t s) {
    if (p->n == 0) return DXO_OK;
    const PmgRun R{ctx, p, s};
    const double* c = p->pairs();
    const int m = p->set_degree;
    int rc;
    // the polynomial from x = 0: the first step needs no product
    R.cheby_first(c, r, p->x);
    for (int k = 1; k < m; ++k) {
        if ((rc = R.op(p->x, p->t)) != DXO_OK) return rc;
        R.cheby(c + 2 * k, r, p->x, p->x);
    }
    // the coarse correction of the residual r - A x
    if ((rc = R.op(p->x, p->t)) != DXO_OK) return rc;
    R.restrict_(r, p->t, p->rc);
    if (p->nc > 0 && (rc = R.coarse(p->rc, p->ec)) != DXO_OK) return rc;
    R.prolong(p->ec, p->x, true);
    // the same polynomial from the corrected x; the last step writes z
    for (int k = 0; k < m; ++k) {
        if ((rc = R.op(p->x, p->t)) != DXO_OK) return rc;
        R.cheby(c + 2 * k, r, p->x, k + 1 == m ? z : p->x);
    }
    return DXO_OK;
}

// ---- C ABI
extern "C" int dxo_pmg_create(dxo_ctx* ctx, int64_t n_nodes, int bs, const dxo_amg_transfer* transfer, const int32_t* constrained,
                              int64_t n_constrained, dxo_pmg** out) {
    if (!ctx || !out) return DXO_E_NULL;
    DXO_LOCK(ctx);
    *out = nullptr;
    const char* who = "dxo_pmg_create";
    auto fail = [&](int code, const char* what) { return fail_who(ctx, code, who, what); };
    if (!transfer || (n_constrained > 0 && !constrained) || !transfer->ptr || !transfer->col || !transfer->w || !transfer->coarse_to_fine)
        return fail(DXO_E_NULL, "NULL argument");
    if (bs < 1 || bs > 3) return fail(DXO_E_DIM, "bs must be 1, 2 or 3");
    if (n_nodes < 0 || n_constrained < 0) return fail(DXO_E_SIZE, "n_nodes < 0 or n_constrained < 0");
    if (n_nodes * bs >= ((int64_t)1 << 31)) return fail(DXO_E_SIZE, "2^31 dofs or more");
    // the transfer, host arrays (pmg_symbolic.h)
    const dxo_amg_transfer& w = *transfer;
    const int64_t n = n_nodes, nc = w.n_coarse;
    {
        const char* what = nullptr;
        const int code = pmg_check_transfer(n, w, &what);
        if (code != DXO_OK) return fail(code, what);
    }
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipStreamSynchronize(s));      // the list may have been written on the stream
    // the constrained dofs (out-of-range entries are ignored)
    const int64_t n_rows = n * bs, pb = w.ptr[n];
    std::vector<uint8_t> mask((size_t)n_rows, 0);
    if (n_constrained > 0) {
        std::vector<int32_t> list((size_t)n_constrained);
        DXO_HIP(ctx, hipMemcpy(list.data(), constrained, list.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t dof : list)
            if (dof >= 0 && dof < n_rows) mask[(size_t)dof] = 1;
    }
    pmg_tables T;
    pmg_build_tables(n, bs, w, mask, T);
    dxo_pmg* p = new dxo_pmg;
    p->device = ctx->device;
    p->bs = bs;
    p->n_nodes = n, p->n = n_rows, p->n_coarse = nc, p->nc = nc * bs, p->p_blocks = pb, p->n_c_bc = (int64_t)T.c_bc.size();
    hipError_t e;
    auto bad = [&](const char* what) {
        pmg_free(p);
        return dxo_hip_fail(ctx, e, what);
    };
    if ((e = pmg_upload(&p->p_ptr, T.p_ptr)) != hipSuccess || (e = pmg_upload(&p->p_col, T.p_col)) != hipSuccess ||
        (e = pmg_upload(&p->p_diag, T.p_diag)) != hipSuccess || (e = pmg_upload(&p->pt_ptr, T.pt_ptr)) != hipSuccess ||
        (e = pmg_upload(&p->pt_blk, T.pt_blk)) != hipSuccess || (e = pmg_upload(&p->pt_row, T.pt_row)) != hipSuccess ||
        (e = pmg_upload(&p->c_bc, T.c_bc)) != hipSuccess)
        return bad("dxo_pmg_create: the transfer");
    if ((e = pmg_zeros(&p->x, n_rows)) != hipSuccess || (e = pmg_zeros(&p->d, n_rows)) != hipSuccess || (e = pmg_zeros(&p->t, n_rows)) != hipSuccess ||
        (e = pmg_zeros(&p->w, n_rows)) != hipSuccess || (e = pmg_zeros(&p->rc, p->nc)) != hipSuccess || (e = pmg_zeros(&p->ec, p->nc)) != hipSuccess ||
        (e = pmg_zeros(&p->part, PMG_MAX_PARTS)) != hipSuccess || (e = pmg_zeros(&p->scal, 4 + 2 * PMG_MAX_DEGREE)) != hipSuccess)
        return bad("dxo_pmg_create: vectors");
    {
        std::lock_guard<std::mutex> g(pmg_live_mu);
        pmg_live.insert(p);
    }
    *out = p;
    return DXO_OK;
}

extern "C" int dxo_pmg_destroy(dxo_ctx* ctx, dxo_pmg* pmg) {
    if (!pmg) return DXO_E_NULL;
    DXO_LOCK(ctx);
    {
        std::lock_guard<std::mutex> g(pmg_live_mu);
        if (!pmg_live.erase(pmg)) return dxo_fail(ctx, DXO_E_OPTION, "dxo_pmg_destroy: not an object of dxo_pmg_create (or destroyed before)");
    }
    (void)hipSetDevice(pmg->device);
    (void)hipDeviceSynchronize();
    pmg_free(pmg);
    return DXO_OK;
}

extern "C" int dxo_pmg_set_smoother(dxo_ctx* ctx, dxo_pmg* pmg, int degree, int rho_iters, double lower, double safety) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!pmg) return dxo_fail(ctx, DXO_E_NULL, "dxo_pmg_set_smoother: NULL argument");
    if (degree < 1 || degree > PMG_MAX_DEGREE || rho_iters < 1 || !(lower > 0.0 && lower < 1.0) || !(safety >= 1.0))
        return dxo_fail(ctx, DXO_E_OPTION, "dxo_pmg_set_smoother: degree must lie in 1..8, rho_iters >= 1, lower in (0, 1), safety >= 1");
    pmg->degree = degree, pmg->rho_iters = rho_iters, pmg->lower = lower, pmg->safety = safety;
    pmg->ready = false;
    return DXO_OK;
}

extern "C" int dxo_pmg_setup(dxo_ctx* ctx, dxo_pmg* pmg, const dxo_krylov_op* fine, const double* dinv, const dxo_krylov_pc* coarse) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    const char* who = "dxo_pmg_setup";
    auto fail = [&](int code, const char* what) { return fail_who(ctx, code, who, what); };
    if (!pmg || !fine || !dinv || !coarse) return fail(DXO_E_NULL, "NULL argument");
    pmg->ready = false;
    if (!fine->csr && !fine->apply) return fail(DXO_E_NULL, "the operator has neither a matrix nor a callback");
    if (fine->csr && !fine->values) return fail(DXO_E_NULL, "the operator's matrix has no values");
    if (fine->n != pmg->n || (fine->csr && fine->csr->n_rows != pmg->n)) return fail(DXO_E_SIZE, "the operator's size is not n_nodes * bs");
    if (fine->csr && fine->csr->bs != pmg->bs) return fail(DXO_E_DIM, "the operator's matrix has another block size");
    if (pmg_misaligned(dinv) || (fine->values && pmg_misaligned(fine->values))) return fail(DXO_E_ALIGN, "arrays must be 8-byte aligned");
    dxo_krylov_callback cb = {};
    switch (coarse->kind) {
    case DXO_PC_AMG:
    case DXO_PC_BLOCK_JACOBI:
    case DXO_PC_JACOBI:
    case DXO_PC_CALLBACK:
        break;
    default:
        return fail(DXO_E_OPTION, "the coarse preconditioner must be DXO_PC_AMG, DXO_PC_BLOCK_JACOBI, DXO_PC_JACOBI or DXO_PC_CALLBACK");
    }
    if (!coarse->inv) return fail(DXO_E_NULL, "the coarse preconditioner carries nothing");
    if (coarse->n != pmg->nc) return fail(DXO_E_SIZE, "the coarse preconditioner does not cover n_coarse * bs rows");
    if (coarse->kind == DXO_PC_AMG) {
        if (coarse->bs != pmg->bs) return fail(DXO_E_DIM, "the coarse multigrid has another block size");
        const int rc = dxo_amg_pc_check(ctx, who, (const dxo_amg*)coarse->inv, nullptr, coarse->bs, coarse->n);
        if (rc != DXO_OK) return rc;
        if (dxo_amg_cycle_is_k((const dxo_amg*)coarse->inv)) return fail(DXO_E_OPTION, "a K-cycle is not a fixed linear operator");
    } else if (coarse->kind == DXO_PC_CALLBACK) {
        cb = *(const dxo_krylov_callback*)coarse->inv;
        if (!cb.apply) return fail(DXO_E_NULL, "the coarse preconditioner has no callback");
    } else {
        if (coarse->kind == DXO_PC_BLOCK_JACOBI && coarse->bs != pmg->bs) return fail(DXO_E_DIM, "the coarse block Jacobi has another block size");
        if (pmg_misaligned(coarse->inv)) return fail(DXO_E_ALIGN, "the coarse inverse is not 8-byte aligned");
    }
    pmg->fine = *fine, pmg->dinv = dinv, pmg->coarse = *coarse, pmg->coarse_cb = cb;
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = dxo_launch_stream(ctx);
    int rc = dxo_device_begin(ctx, s);
    if (rc != DXO_OK) return rc;
    // rho of Dinv A by the power iteration, then the pairs: all on the device
    const PmgRun R{ctx, pmg, s};
    const int64_t n = pmg->n;
    const int nb = pmg_parts(n);
    const dim3 B(PMG_BLOCK);
    hipLaunchKernelGGL(pmg_power_init, dim3(nb), B, 0, s, n, pmg->w, pmg->part);
    hipLaunchKernelGGL(pmg_power_norm, dim3(1), B, 0, s, pmg->part, nb, 0, pmg->safety, pmg->lower, pmg->degree, pmg->scal);
    for (int it = 0; it < pmg->rho_iters; ++it) {
        hipLaunchKernelGGL(pmg_scale, pmg_grid(ctx, n), B, 0, s, n, pmg->scal, pmg->w, pmg->t);
        if (n > 0 && (rc = R.op(pmg->t, pmg->x)) != DXO_OK) return rc;
        hipLaunchKernelGGL(pmg_dinv_norm, dim3(nb), B, 0, s, n, dinv, pmg->x, pmg->w, pmg->part);
        hipLaunchKernelGGL(pmg_power_norm, dim3(1), B, 0, s, pmg->part, nb, it + 1 == pmg->rho_iters ? 1 : 0, pmg->safety, pmg->lower, pmg->degree,
                           pmg->scal);
    }
    pmg->set_degree = pmg->degree;
    rc = dxo_device_end(ctx, s);
    if (rc != DXO_OK) return rc;
    pmg->ready = true;
    return DXO_OK;
}

extern "C" int dxo_pmg_apply(dxo_ctx* ctx, dxo_pmg* pmg, const double* r, double* z) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    int rc = pmg_check_vectors(ctx, "dxo_pmg_apply", pmg, r, z);
    if (rc != DXO_OK) return rc;
    if (!pmg->ready) return dxo_fail(ctx, DXO_E_OPTION, "dxo_pmg_apply: dxo_pmg_setup has not run (or failed, or dxo_pmg_set_smoother came after it)");
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = dxo_device_begin(ctx, s)) != DXO_OK) return rc;
    rc = dxo_pmg_cycle(ctx, pmg, r, z, s);
    const int end = dxo_device_end(ctx, s);
    return rc != DXO_OK ? rc : end;
}

extern "C" int dxo_pmg_restrict(dxo_ctx* ctx, dxo_pmg* pmg, const double* r_fine, double* r_coarse) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    int rc = pmg_check_vectors(ctx, "dxo_pmg_restrict", pmg, r_fine, r_coarse);
    if (rc != DXO_OK) return rc;
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = dxo_device_begin(ctx, s)) != DXO_OK) return rc;
    PmgRun{ctx, pmg, s}.restrict_(r_fine, nullptr, r_coarse);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_pmg_prolong(dxo_ctx* ctx, dxo_pmg* pmg, const double* e_coarse, double* x_fine) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    int rc = pmg_check_vectors(ctx, "dxo_pmg_prolong", pmg, e_coarse, x_fine);
    if (rc != DXO_OK) return rc;
    hipStream_t s = dxo_launch_stream(ctx);
    DXO_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = dxo_device_begin(ctx, s)) != DXO_OK) return rc;
    PmgRun{ctx, pmg, s}.prolong(e_coarse, x_fine, false);
    return dxo_device_end(ctx, s);
}

extern "C" int dxo_pmg_info(dxo_ctx* ctx, const dxo_pmg* pmg, int64_t* n_coarse_rows, int64_t* p_blocks, const double** p_diag,
                            const int32_t** coarse_constrained, int64_t* n_coarse_constrained, const double** rho, const double** pairs, int* degree,
                            int64_t* matvecs_per_apply) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!pmg) return dxo_fail(ctx, DXO_E_NULL, "dxo_pmg_info: NULL argument");
    if (n_coarse_rows) *n_coarse_rows = pmg->nc;
    if (p_blocks) *p_blocks = pmg->p_blocks;
    if (p_diag) *p_diag = pmg->p_diag;
    if (coarse_constrained) *coarse_constrained = pmg->c_bc;
    if (n_coarse_constrained) *n_coarse_constrained = pmg->n_c_bc;
    if (rho) *rho = pmg->rho();
    if (pairs) *pairs = pmg->pairs();
    if (degree) *degree = pmg->degree;
    if (matvecs_per_apply) *matvecs_per_apply = 2 * (int64_t)pmg->degree;
    return DXO_OK;
}
