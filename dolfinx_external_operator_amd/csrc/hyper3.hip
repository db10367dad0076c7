// hyper3.hip — the analytic Isihara model for a 3x3 deformation gradient (hyper3_core.h): dxo_isihara3 over an array of F, and
// dxo_isihara3_field with F = I + grad u formed in the registers of the same kernel from the dof vector of a gdim = 3 mesh. The 3-D
// twins of isihara_tile (icnn.hip) and isihara_field (field_ops.hip): lane = point, results staged in the wave's LDS slice, stores in
// output order. Both are HBM-bound: 72 B in (plain) and 720 B out per point.
//
// LDS: a wave's full tile would be 64 x 90 doubles = 45 KiB, four of them 180 KiB. The tangent therefore leaves in passes of `pp`
// points — a run of pp * 81 consecutive doubles, so every store instruction but a run's last still covers 1 KiB of consecutive
// addresses — while the 45 unique entries of every lane wait in registers; the stresses follow as one run. pp = 16 in the plain
// kernel: 10.1 KiB per wave, 40.6 KiB per workgroup; registers allow two workgroups per compute unit (H3_WAVES). The field kernel shares its 64 KiB with the
// element tables (40 KiB for Q2 hexahedra under the 27-point rule) and takes the largest pp <= 16 that fits; every mesh
// dxo_mesh_create accepts leaves room for pp >= 9.
#include "dxo_common.h"
#include "hyper3_core.h"
#include "hyper_host.h"

namespace {

// waves per SIMD the kernels are compiled for: a lane holds its point's 45 entries (90 registers) through the passes, next to the
// inputs of the entries still to come: 176 registers in the plain kernel, 244 in the field kernel, no scratch. Compiled for three
// waves (168 registers) they spill 28 and 184 bytes per lane (profiles/hyper3_resources.txt)
constexpr int H3_WAVES = 2;
constexpr int H3_PP = 16;                                         // points per tangent pass
__host__ __device__ constexpr int h3_buf(int pp) { return (pp * 81 + 2 + 1) & ~1; }   // doubles of a wave's staging buffer

// one wave tile: the stress is formed, staged and stored first, so its registers are free again while the 45 tangent entries wait
// for their passes
template <bool NT>
__device__ __forceinline__ void h3_point_out(const IsiPrm& prm, const double (&Fv)[9], double* X, int pp, int lane, int npts,
                                             double* __restrict__ dP, double* __restrict__ P) {
    Isi3Point q;
    {
        double Pv[9];
        isihara3_stress(prm, Fv, q, Pv);
        hyper3_store_stress<NT>(X, lane, npts, Pv, P);
    }
    double H[HYPER3_SYM];
    isihara3_tangent(q, H);
    hyper3_store_tangent<NT>(X, pp, lane, npts, H, dP);
}

template <bool NT>
__global__ __launch_bounds__(DXO_BLOCK, H3_WAVES) void isihara3_tile(IsiPrm prm, int64_t n, const double* __restrict__ F,
                                                           double* __restrict__ dP, double* __restrict__ P) {
    constexpr int WAVES = DXO_BLOCK / DXO_WAVE;
    __shared__ __attribute__((aligned(16))) double lds[WAVES * h3_buf(H3_PP)];
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: tile indices and base pointers stay in scalar registers
    double* X = lds + wave * h3_buf(H3_PP);
    const int64_t n_tiles = (n + DXO_WAVE - 1) / DXO_WAVE;
    const int64_t tile_stride = (int64_t)gridDim.x * WAVES;
    for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < n_tiles; tile += tile_stride) {
        const int64_t p0 = tile * DXO_WAVE;
        const int npts = (n - p0 < DXO_WAVE) ? (int)(n - p0) : DXO_WAVE;
        double Fv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        if (lane < npts) {
#pragma unroll
            for (int k = 0; k < 9; ++k) Fv[k] = F[(p0 + lane) * 9 + k];
        }
        h3_point_out<NT>(prm, Fv, X, H3_PP, lane, npts, dP + p0 * 81, P + p0 * 9);
    }
}

int isihara3_launch(dxo_ctx* ctx, const IsiPrm& prm, int64_t n, const double* F, double* dP, double* P, hipStream_t s) {
    if (n == 0) return DXO_OK;
    const int64_t n_tiles = (n + DXO_WAVE - 1) / DXO_WAVE;
    const int grid = dxo_grid_for_tiles(ctx, n_tiles, DXO_BLOCK / DXO_WAVE);
    if (ctx->nontemporal != 0) hipLaunchKernelGGL(isihara3_tile<true>, dim3(grid), dim3(DXO_BLOCK), 0, s, prm, n, F, dP, P);
    else hipLaunchKernelGGL(isihara3_tile<false>, dim3(grid), dim3(DXO_BLOCK), 0, s, prm, n, F, dP, P);
    return DXO_OK;
}

int isihara3_chunk(dxo_ctx* ctx, void* user, int64_t m, void* const* d_in, void* const* d_out, hipStream_t s) {
    return isihara3_launch(ctx, *static_cast<const IsiPrm*>(user), m, (const double*)d_in[0], (double*)d_out[0], (double*)d_out[1], s);
}

// ---- the operand in registers: a wave owns floor(64 / nq) consecutive cells, each lane forms F = I + grad u of its own quadrature point
// (operand_core.h) and evaluates the model; the gather buffer, free again after the contraction, is the staging buffer of the stores.
template <bool NT>
__global__ __launch_bounds__(DXO_BLOCK, H3_WAVES) void isihara3_field(IsiPrm prm, OperandDev m, int wave_doubles, int pp, int64_t cell0, int64_t n_cells,
                                                            const double* __restrict__ u, double* __restrict__ dP,
                                                            double* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* tab = lds;
    operand_load_tables<3>(m, tab);
    __syncthreads();
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: tile indices and base pointers stay in scalar registers
    double* W = lds + m.table_doubles + wave * wave_doubles;
    const int cpw = m.cells_per_wave;
    const int64_t n_groups = (n_cells + cpw - 1) / cpw;
    const GroupWalk walk = xcd_group_walk(n_groups, DXO_BLOCK / DXO_WAVE, wave);
    for (int64_t grp = walk.first; grp < walk.end; grp += walk.stride) {
        const int64_t c0 = grp * cpw;
        const int ncell = (n_cells - c0 < cpw) ? (int)(n_cells - c0) : cpw;
        const int npts = ncell * m.nq;
        const int64_t p0 = c0 * m.nq;
        double Fv[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        operand_point<3, 3, DXO_OPERAND_DEFGRAD>(m, tab, W, u, nullptr, cell0 + c0, ncell, lane, Fv);
        h3_point_out<NT>(prm, Fv, W, pp, lane, npts, dP + p0 * 81, P + p0 * 9);      // lanes without a point evaluate the identity and store nothing
    }
}

int isi3_field_launch(dxo_ctx* ctx, const IsiFieldLaunch& L, int64_t cell0, int64_t n_cells, double* dP, double* P, hipStream_t s) {
    if (n_cells == 0) return DXO_OK;
    const OperandDev& m = L.mesh->dev;
    // the largest pass that fits beside the tables; dxo_mesh_create keeps 64 * 12 doubles per wave free, more than h3_buf(9)
    const int room = ((64 * 1024 / (int)sizeof(double) - m.table_doubles) / 4) & ~1;
    int pp = (room - 2) / 81;
    if (pp > H3_PP) pp = H3_PP;
    if (pp < 8 || room < m.wave_doubles) return dxo_fail(ctx, DXO_E_SIZE, "dxo_isihara3_field: element too large for the LDS budget");
    const int wd = std::max(m.wave_doubles, h3_buf(pp));
    const size_t shm = (size_t)(m.table_doubles + 4 * wd) * sizeof(double);
    const int blocks = wave_group_grid(ctx, wave_groups(m, n_cells), 4);
    if (ctx->nontemporal != 0) hipLaunchKernelGGL(isihara3_field<true>, dim3(blocks), dim3(DXO_BLOCK), shm, s, L.prm, m, wd, pp, cell0, n_cells, L.d_u, dP, P);
    else hipLaunchKernelGGL(isihara3_field<false>, dim3(blocks), dim3(DXO_BLOCK), shm, s, L.prm, m, wd, pp, cell0, n_cells, L.d_u, dP, P);
    return DXO_OK;
}

}  // namespace

extern "C" int dxo_isihara3(dxo_ctx* ctx, const dxo_isihara_params* prm, int64_t n, int mem, const double* F, double* dP,
                            double* P) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!prm) return dxo_fail(ctx, DXO_E_NULL, "dxo_isihara3: params is NULL");
    IsiPrm k{prm->c1, prm->c2, prm->c3, prm->c4};
    return hyper_array_entry(ctx, "dxo_isihara3", n, mem, F, dP, P, 3, isihara3_chunk, &k, true);
}

extern "C" int dxo_isihara3_field(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, int mem, const double* u,
                                  double* dP, double* P) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!prm) return dxo_fail(ctx, DXO_E_NULL, "dxo_isihara3_field: params is NULL");
    const int rc = hyper_field_check(ctx, "dxo_isihara3_field", 3, mesh, mem, u, dP, P);
    if (rc != DXO_OK || mesh->num_cells == 0) return rc;
    return isi_field_run(ctx, IsiFieldLaunch{IsiPrm{prm->c1, prm->c2, prm->c3, prm->c4}, mesh, u, isi3_field_launch}, 3, mem, dP, P);
}
