// mohr_coulomb3.hip — Mohr-Coulomb (Abbo-Sloan) return mapping and forward-mode-through-Newton tangent on the six-component
// Mandel strain (xx, yy, zz, sqrt2 xy, sqrt2 xz, sqrt2 yz): the 3-D form of mohr_coulomb.hip. The per-point algorithm is
// csrc/mc3_core.h.
//
// Traffic: 432 B per point (12 doubles in, 36 + 6 out; + 28 B with the four diagnostics) against several kflop of fp64 per
// Newton pass: fp64-VALU- and divergence-bound on plastic points, HBM-bound on elastic ones. So the work is split as in the
// classify + Newton form of the 2-D operator:
//   mc3_classify  lane = point, HBM-bound, four waves per workgroup: trial stress, f(trial). Elastic points are finished here —
//                 C_elas from constants in output order, sigma through the wave's LDS slice, both with masked 16-byte stores.
//                 Plastic points go on a compact index list (one atomic per ~512 of them and wave).
//   mc3_newton    fp64-bound, ONE wave per workgroup: a lane takes a point from the list, keeps it until cond_fun fails, writes
//                 its rows once and is refilled while its neighbours iterate, so every pass runs on nearly full waves.
// Why two kernels and one-wave workgroups ("3-D Mohr-Coulomb"): a lane's parked state — deps[6], sn[6], Y[7][6] — is
// 54 doubles, 27 KiB per wave in the slot-major, lane-minor layout; five such waves would fit the 160 KiB of a CU, but the pass
// itself holds 294 registers with that state parked (bounded to 256 it keeps 144 B of scratch per lane), so the Newton kernel runs
// one wave per SIMD, four one-wave workgroups per CU, without scratch. The classification needs neither that LDS nor those
// registers and runs at four waves per SIMD; fused into the Newton kernel it would stream 432 B per point through four waves per CU.
//   mc3_point     the cross-check form (ctx option mc_variant = 0): lane = point, every lane iterates its own point to the end
//                 on the same lane math and the same LDS layout; bit-identical outputs.
#include "dxo_common.h"
#include "mc3_core.h"

namespace {

constexpr int MC3_PENDING = 512;   // per-wave buffer of plastic point indices (mc3_classify)
constexpr int MC3_BATCH = 256;     // list entries a wave reserves per cursor atomic (mc3_newton)
constexpr int MC3_SLOTS = 54;      // LDS doubles per lane: deps[6], sn[6], Y[7][6]
constexpr int MC3_WAVES_PER_CU = 4;  // one per SIMD: the pass holds 294 registers (256 + 38 accumulation registers, no scratch)

__device__ __forceinline__ void st16nt(dxo_f64x2* p, dxo_f64x2 v) { __builtin_nontemporal_store(v, p); }

// slot-major, lane-minor (a slot of all 64 lanes is 512 contiguous bytes: conflict-free ds_read/write_b64):
// slots 0-5 = deps, 6-11 = sn, 12 + 7 m + i = Y[i][m]
struct LaneLds3 {
    double* slots;   // wave slice + lane
    __device__ __forceinline__ void set_inputs(const double* d, const double* s) {
#pragma unroll
        for (int i = 0; i < 6; ++i) { slots[i * DXO_WAVE] = d[i]; slots[(6 + i) * DXO_WAVE] = s[i]; }
    }
    __device__ __forceinline__ void get_inputs(double* d, double* s) const {
#pragma unroll
        for (int i = 0; i < 6; ++i) { d[i] = slots[i * DXO_WAVE]; s[i] = slots[(6 + i) * DXO_WAVE]; }
    }
    __device__ __forceinline__ void get_col(int m, double* v7) const {
#pragma unroll
        for (int i = 0; i < 7; ++i) v7[i] = slots[(12 + 7 * m + i) * DXO_WAVE];
    }
    __device__ __forceinline__ void set_col(int m, const double* v7) {
#pragma unroll
        for (int i = 0; i < 7; ++i) slots[(12 + 7 * m + i) * DXO_WAVE] = v7[i];
    }
};
using Lane3 = mc3::LaneT<LaneLds3>;

__device__ __forceinline__ void mc3_load_point(const double* __restrict__ deps, const double* __restrict__ sigma_n, int64_t i, double* e,
                                               double* sn) {
    const dxo_f64x2* ge = reinterpret_cast<const dxo_f64x2*>(deps + i * 6);
    const dxo_f64x2* gs = reinterpret_cast<const dxo_f64x2*>(sigma_n + i * 6);
    const dxo_f64x2 e0 = ge[0], e1 = ge[1], e2 = ge[2], s0 = gs[0], s1 = gs[1], s2 = gs[2];
    e[0] = e0.x; e[1] = e0.y; e[2] = e1.x; e[3] = e1.y; e[4] = e2.x; e[5] = e2.y;
    sn[0] = s0.x; sn[1] = s0.y; sn[2] = s1.x; sn[3] = s1.y; sn[4] = s2.x; sn[5] = s2.y;
}

// a finished plastic point: its 6 x 6 rows (C_tang[r][c] = Y[r][c], read back from the lane's LDS slots), its stress and diagnostics
__device__ __forceinline__ void mc3_store_point(const Lane3& L, int64_t idx, double* __restrict__ C_tang, double* __restrict__ sigma,
                                                int32_t* __restrict__ niter, double* __restrict__ norm_res, double* __restrict__ dlambda) {
    dxo_f64x2* gc = reinterpret_cast<dxo_f64x2*>(C_tang + idx * 36);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            gc[3 * r + c] = dxo_f64x2{L.st.slots[(12 + 7 * (2 * c) + r) * DXO_WAVE], L.st.slots[(12 + 7 * (2 * c + 1) + r) * DXO_WAVE]};
    }
    dxo_f64x2* gg = reinterpret_cast<dxo_f64x2*>(sigma + idx * 6);
    gg[0] = dxo_f64x2{L.sig[0], L.sig[1]};
    gg[1] = dxo_f64x2{L.sig[2], L.sig[3]};
    gg[2] = dxo_f64x2{L.sig[4], L.sig[5]};
    if (niter) niter[idx] = L.niter;
    if (norm_res) norm_res[idx] = L.norm;
    if (dlambda) dlambda[idx] = L.dl;
}

// ------------------------------------------------------------------ cross-check form: lane = point
template <bool SAME>
__global__ __launch_bounds__(DXO_WAVE) void mc3_point(mc::Const k, int64_t n, const double* __restrict__ deps,
                                                      const double* __restrict__ sigma_n, double* __restrict__ C_tang,
                                                      double* __restrict__ sigma, int32_t* __restrict__ niter,
                                                      double* __restrict__ yielding, double* __restrict__ norm_res,
                                                      double* __restrict__ dlambda) {
    __shared__ double lane_state[MC3_SLOTS * DXO_WAVE];
    const int lane = threadIdx.x;
    Lane3 L;
    L.st.slots = lane_state + lane;
    const int64_t n_tiles = (n + DXO_WAVE - 1) / DXO_WAVE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t i = tile * DXO_WAVE + lane;
        if (i >= n) continue;
        double e[6], sn[6], Ce[6], trial[6];
        mc3_load_point(deps, sigma_n, i, e, sn);
        mc3::C_times(k, e, Ce);
#pragma unroll
        for (int c = 0; c < 6; ++c) trial[c] = sn[c] + Ce[c];
        const double yld = mc3::f_value(k, trial, SAME ? 1 : 0);
        if (yielding) yielding[i] = yld;
        if (yld <= 0.0) {                                   // NaN -> plastic branch, as lax.cond does
            double sg[6], nr;
            int32_t it;
            mc3::elastic_sigma(k, sn, Ce, trial, sg, it, nr);
            dxo_f64x2* gc = reinterpret_cast<dxo_f64x2*>(C_tang + i * 36);
#pragma unroll
            for (int r = 0; r < 6; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    dxo_f64x2 v{mc3::c_elas_entry(k, r, 2 * c), mc3::c_elas_entry(k, r, 2 * c + 1)};
                    if (it == 0) v = dxo_f64x2{0.0, 0.0};
                    gc[3 * r + c] = v;
                }
            }
            dxo_f64x2* gg = reinterpret_cast<dxo_f64x2*>(sigma + i * 6);
            gg[0] = dxo_f64x2{sg[0], sg[1]};
            gg[1] = dxo_f64x2{sg[2], sg[3]};
            gg[2] = dxo_f64x2{sg[4], sg[5]};
            if (niter) niter[i] = it;
            if (norm_res) norm_res[i] = nr;
            if (dlambda) dlambda[i] = 0.0;
        } else {
            mc3::lane_init(L, e, sn);
            while (!mc3::lane_pass<SAME>(k, L)) {}
            mc3_store_point(L, i, C_tang, sigma, niter, norm_res, dlambda);
        }
    }
}

// ------------------------------------------------------------------ production form: classify + compacted Newton
// Scratch (ctx-owned): header {uint32 n_plastic, uint32 cursor} + int32 list[points of the part].
struct Mc3ScratchHeader {
    unsigned int n_plastic;
    unsigned int cursor;
    unsigned int pad[62];
};

__global__ __launch_bounds__(DXO_BLOCK) void mc3_classify(mc::Const k, int64_t n, const double* __restrict__ deps,
                                                          const double* __restrict__ sigma_n, double* __restrict__ C_tang,
                                                          double* __restrict__ sigma, int32_t* __restrict__ niter,
                                                          double* __restrict__ yielding, double* __restrict__ norm_res,
                                                          double* __restrict__ dlambda, Mc3ScratchHeader* __restrict__ hdr,
                                                          int32_t* __restrict__ list) {
    constexpr int WAVES = DXO_BLOCK / DXO_WAVE;
    __shared__ __attribute__((aligned(16))) double lds[WAVES * DXO_WAVE * 6];
    __shared__ int32_t pending[WAVES * MC3_PENDING];
    const int lane = threadIdx.x & (DXO_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    dxo_f64x2* X2 = reinterpret_cast<dxo_f64x2*>(lds + wave * (DXO_WAVE * 6));
    int32_t* pend = pending + wave * MC3_PENDING;
    int n_pend = 0;                                    // wave-uniform
    auto flush = [&]() {
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(&hdr->n_plastic, (unsigned int)n_pend);
        base = __builtin_amdgcn_readfirstlane(base);
        for (int j = lane; j < n_pend; j += DXO_WAVE) list[base + j] = pend[j];
        n_pend = 0;
    };
    const int64_t n_tiles = (n + DXO_WAVE - 1) / DXO_WAVE;
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    for (int64_t tile = (int64_t)blockIdx.x * WAVES + wave; tile < n_tiles; tile += stride) {
        const int64_t p0 = tile * DXO_WAVE;
        const int npts = (n - p0 < DXO_WAVE) ? (int)(n - p0) : DXO_WAVE;
        const bool live = lane < npts;
        const int64_t i = p0 + (live ? lane : 0);
        double e[6], sn[6], Ce[6], trial[6];
        mc3_load_point(deps, sigma_n, i, e, sn);
        mc3::C_times(k, e, Ce);
#pragma unroll
        for (int c = 0; c < 6; ++c) trial[c] = sn[c] + Ce[c];
        const double yld = mc3::f_value(k, trial, k.same_angle ? 1 : 0);
        const bool elastic = yld <= 0.0;               // NaN -> plastic branch
        double sg[6], nr;
        int32_t it;
        mc3::elastic_sigma(k, sn, Ce, trial, sg, it, nr);
        const unsigned long long el_mask = __ballot(live && elastic);
        const unsigned long long zero_mask = __ballot(live && elastic && it == 0);
        const unsigned long long pl_mask = __ballot(live && !elastic);
        if (pl_mask) {
            if (n_pend + DXO_WAVE > MC3_PENDING) flush();
            if (live && !elastic) pend[n_pend + __popcll(pl_mask & ((1ull << lane) - 1ull))] = (int32_t)i;
            n_pend += __popcll(pl_mask);
        }
        if (live) {
            if (yielding) yielding[i] = yld;
            if (elastic) {
                if (niter) niter[i] = it;
                if (norm_res) norm_res[i] = nr;
                if (dlambda) dlambda[i] = 0.0;
            }
        }
        // sigma of elastic points: point-per-lane rows -> lane-linear 16-byte stores, masked by the owner's branch (a plastic
        // point's rows are written once, by its Newton lane)
        X2[lane * 3] = dxo_f64x2{sg[0], sg[1]};
        X2[lane * 3 + 1] = dxo_f64x2{sg[2], sg[3]};
        X2[lane * 3 + 2] = dxo_f64x2{sg[4], sg[5]};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        dxo_f64x2* gg = reinterpret_cast<dxo_f64x2*>(sigma + p0 * 6);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int q = t * DXO_WAVE + lane;
            if ((el_mask >> (q / 3)) & 1ull) st16nt(gg + q, X2[q]);
        }
        // C_tang of elastic points: constants in output order (chunk q = point q / 18, row (q % 18) / 3, columns 2 (q % 3), + 1)
        dxo_f64x2* gc = reinterpret_cast<dxo_f64x2*>(C_tang + p0 * 36);
#pragma unroll 2
        for (int t = 0; t < 18; ++t) {
            const int q = t * DXO_WAVE + lane;
            const int pt = q / 18, c = q - pt * 18;
            const int row = c / 3, col = (c - row * 3) * 2;
            dxo_f64x2 v;
            v.x = ((row < 3 && col < 3) ? k.lmbda : 0.0) + (row == col ? k.mu2 : 0.0);
            v.y = ((row < 3 && col + 1 < 3) ? k.lmbda : 0.0) + (row == col + 1 ? k.mu2 : 0.0);
            if ((zero_mask >> pt) & 1ull) v = dxo_f64x2{0.0, 0.0};
            if ((el_mask >> pt) & 1ull) st16nt(gc + q, v);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (n_pend) flush();
}

template <bool SAME>
__global__ __launch_bounds__(DXO_WAVE) void mc3_newton(mc::Const k, const double* __restrict__ deps, const double* __restrict__ sigma_n,
                                                       double* __restrict__ C_tang, double* __restrict__ sigma,
                                                       int32_t* __restrict__ niter, double* __restrict__ norm_res,
                                                       double* __restrict__ dlambda, Mc3ScratchHeader* __restrict__ hdr,
                                                       const int32_t* __restrict__ list) {
    __shared__ double lane_state[MC3_SLOTS * DXO_WAVE];
    const int lane = threadIdx.x;
    const unsigned int total = hdr->n_plastic;   // written by mc3_classify, earlier on the same stream
    Lane3 L;
    L.st.slots = lane_state + lane;
    bool active = false, exhausted = false;
    int64_t idx = 0;
    unsigned int lo = 0, hi = 0;   // the wave's reserved slice of the list (wave-uniform)
    for (;;) {
        const unsigned long long idle = __ballot(!active);
        if (idle && lo == hi && !exhausted) {
            unsigned int start = 0;
            if (lane == 0) start = atomicAdd(&hdr->cursor, (unsigned int)MC3_BATCH);
            start = __builtin_amdgcn_readfirstlane(start);
            if (start >= total) exhausted = true;
            else { lo = start; hi = (start + MC3_BATCH < total) ? start + MC3_BATCH : total; }
        }
        if (idle && lo < hi) {
            const unsigned int mine = lo + (unsigned int)__popcll(idle & ((1ull << lane) - 1ull));
            const unsigned int take = ((unsigned int)__popcll(idle) < hi - lo) ? (unsigned int)__popcll(idle) : hi - lo;
            lo += take;
            if (!active && mine < hi) {
                idx = list[mine];
                double e[6], sn[6];
                mc3_load_point(deps, sigma_n, idx, e, sn);
                mc3::lane_init(L, e, sn);
                active = true;
            }
        }
        if (!__ballot(active)) break;
        if (active) {
            if (mc3::lane_pass<SAME>(k, L)) {
                mc3_store_point(L, idx, C_tang, sigma, niter, norm_res, dlambda);
                active = false;
            }
        }
    }
}

struct Mc3Launch {
    mc::Const k;
    bool d_niter, d_yield, d_res, d_dl;
};

int mc3_launch(dxo_ctx* ctx, const Mc3Launch& L, int64_t n, const double* deps, const double* sigma_n, double* C_tang, double* sigma,
               int32_t* niter, double* yielding, double* norm_res, double* dlambda, hipStream_t s) {
    if (n == 0) return DXO_OK;
    const bool same = L.k.same_angle != 0;
    if (ctx->mc_variant == 0) {
        const int64_t n_tiles = (n + DXO_WAVE - 1) / DXO_WAVE;
        const int grid = dxo_grid_for_tiles(ctx, n_tiles, 1);
        if (same) hipLaunchKernelGGL(mc3_point<true>, dim3(grid), dim3(DXO_WAVE), 0, s, L.k, n, deps, sigma_n, C_tang, sigma, niter, yielding, norm_res, dlambda);
        else hipLaunchKernelGGL(mc3_point<false>, dim3(grid), dim3(DXO_WAVE), 0, s, L.k, n, deps, sigma_n, C_tang, sigma, niter, yielding, norm_res, dlambda);
        DXO_HIP(ctx, hipGetLastError());
        return DXO_OK;
    }
    // int32 list entries: split gigantic batches (and whatever the option mc_part_points asks for)
    int64_t max_part = ctx->mc_part_points;
    if (max_part < DXO_WAVE) max_part = DXO_WAVE;
    if (max_part > ((int64_t)1 << 30)) max_part = (int64_t)1 << 30;
    max_part = max_part / DXO_WAVE * DXO_WAVE;      // parts start on 16-byte aligned rows
    for (int64_t off = 0; off < n; off += max_part) {
        const int64_t m = (n - off < max_part) ? (n - off) : max_part;
        void* scratch = dxo_scratch(ctx, s, sizeof(Mc3ScratchHeader) + (size_t)m * sizeof(int32_t));
        if (!scratch) return dxo_hip_fail(ctx, hipErrorOutOfMemory, "dxo_mohr_coulomb3: scratch allocation");
        Mc3ScratchHeader* hdr = static_cast<Mc3ScratchHeader*>(scratch);
        int32_t* list = reinterpret_cast<int32_t*>(hdr + 1);
        DXO_HIP(ctx, hipMemsetAsync(hdr, 0, sizeof(Mc3ScratchHeader), s));
        int64_t cgrid = (m + DXO_BLOCK - 1) / DXO_BLOCK;
        const int64_t ccap = (int64_t)ctx->compute_units * 6;
        if (cgrid > ccap) cgrid = ccap;
        int32_t* it = niter ? niter + off : nullptr;
        double* yl = yielding ? yielding + off : nullptr;
        double* nr = norm_res ? norm_res + off : nullptr;
        double* dl = dlambda ? dlambda + off : nullptr;
        hipLaunchKernelGGL(mc3_classify, dim3((int)cgrid), dim3(DXO_BLOCK), 0, s, L.k, m, deps + off * 6, sigma_n + off * 6, C_tang + off * 36,
                           sigma + off * 6, it, yl, nr, dl, hdr, list);
        int64_t nblocks = (int64_t)ctx->compute_units * MC3_WAVES_PER_CU;
        const int64_t enough = (m + DXO_WAVE - 1) / DXO_WAVE;
        if (nblocks > enough) nblocks = enough;
        if (same) hipLaunchKernelGGL(mc3_newton<true>, dim3((int)nblocks), dim3(DXO_WAVE), 0, s, L.k, deps + off * 6, sigma_n + off * 6, C_tang + off * 36,
                                     sigma + off * 6, it, nr, dl, hdr, list);
        else hipLaunchKernelGGL(mc3_newton<false>, dim3((int)nblocks), dim3(DXO_WAVE), 0, s, L.k, deps + off * 6, sigma_n + off * 6, C_tang + off * 36,
                                sigma + off * 6, it, nr, dl, hdr, list);
        DXO_HIP(ctx, hipGetLastError());
    }
    return DXO_OK;
}

int mc3_chunk(dxo_ctx* ctx, void* user, int64_t m, void* const* d_in, void* const* d_out, hipStream_t s) {
    const Mc3Launch& L = *static_cast<const Mc3Launch*>(user);
    int o = 2;
    int32_t* it = L.d_niter ? (int32_t*)d_out[o++] : nullptr;
    double* yl = L.d_yield ? (double*)d_out[o++] : nullptr;
    double* nr = L.d_res ? (double*)d_out[o++] : nullptr;
    double* dl = L.d_dl ? (double*)d_out[o++] : nullptr;
    return mc3_launch(ctx, L, m, (const double*)d_in[0], (const double*)d_in[1], (double*)d_out[0], (double*)d_out[1], it, yl, nr, dl, s);
}

Mc3Launch mc3_make_launch(const dxo_mc_params* prm, const int32_t* niter, const double* yielding, const double* norm_res, const double* dlambda) {
    return Mc3Launch{mc::make_const(prm->E, prm->nu, prm->c, prm->phi, prm->psi, prm->theta_T, prm->a, prm->tol, prm->nitermax),
                     niter != nullptr, yielding != nullptr, norm_res != nullptr, dlambda != nullptr};
}

}  // namespace

extern "C" int dxo_mohr_coulomb3(dxo_ctx* ctx, const dxo_mc_params* prm, int64_t n, int mem, const double* deps, const double* sigma_n,
                                 double* C_tang, double* sigma, int32_t* niter, double* yielding, double* norm_res, double* dlambda) {
    if (!ctx) return DXO_E_NULL;
    DXO_LOCK(ctx);
    if (!prm) return dxo_fail(ctx, DXO_E_NULL, "dxo_mohr_coulomb3: params is NULL");
    if (n < 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_mohr_coulomb3: n < 0");
    if (mem != DXO_MEM_HOST && mem != DXO_MEM_DEVICE) return dxo_fail(ctx, DXO_E_MEM, "dxo_mohr_coulomb3: bad mem");
    if (n > 0 && (!deps || !sigma_n || !C_tang || !sigma)) return dxo_fail(ctx, DXO_E_NULL, "dxo_mohr_coulomb3: NULL array");
    if (prm->nitermax < 0) return dxo_fail(ctx, DXO_E_SIZE, "dxo_mohr_coulomb3: nitermax < 0");
    int rc = dxo_mc_check_align(ctx, "dxo_mohr_coulomb3", mem, (uintptr_t)deps | (uintptr_t)sigma_n | (uintptr_t)C_tang | (uintptr_t)sigma,
                                "deps/sigma_n/C_tang/sigma must be 16-byte aligned", (uintptr_t)yielding | (uintptr_t)norm_res | (uintptr_t)dlambda, niter);
    if (rc != DXO_OK) return rc;
    Mc3Launch L = mc3_make_launch(prm, niter, yielding, norm_res, dlambda);
    if (mem == DXO_MEM_DEVICE) {
        DXO_HIP(ctx, hipSetDevice(ctx->device));
        hipStream_t s = dxo_launch_stream(ctx);
        rc = dxo_device_begin(ctx, s);
        if (rc != DXO_OK) return rc;
        rc = mc3_launch(ctx, L, n, deps, sigma_n, C_tang, sigma, niter, yielding, norm_res, dlambda, s);
        if (rc != DXO_OK) return rc;
        return dxo_device_end(ctx, s);
    }
    const size_t sd = sizeof(double);
    std::vector<dxo_span> in = {{deps, nullptr, 6 * sd}, {sigma_n, nullptr, 6 * sd}};
    std::vector<dxo_span> out = {{nullptr, C_tang, 36 * sd}, {nullptr, sigma, 6 * sd}};
    dxo_mc_optional_outputs(out, 1, niter, yielding, norm_res, dlambda);
    return dxo_run_host_pipeline(ctx, n, in, out, mc3_chunk, &L);
}

// internal: the kernels on device pointers and an explicit stream (field_ops.hip)
int dxo_mc3_launch_device(dxo_ctx* ctx, const dxo_mc_params* prm, int64_t n, const double* deps, const double* sigma_n, double* C_tang,
                          double* sigma, int32_t* niter, double* yielding, double* norm_res, double* dlambda, hipStream_t s) {
    return mc3_launch(ctx, mc3_make_launch(prm, niter, yielding, norm_res, dlambda), n, deps, sigma_n, C_tang, sigma, niter, yielding, norm_res, dlambda, s);
}
