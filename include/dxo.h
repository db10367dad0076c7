/*
 * dxo.h — C ABI of libdxo_hip.so: MI355X (gfx950) quadrature-point kernels that stand
 * behind dolfinx-external-operator's `external_function(derivatives)(*operand_arrays)`
 * callback (reference: src/dolfinx_external_operator/external_operator.py:432).
 *
 * Every entry point is plain C: pointers, sizes, POD parameter structs. No torch / numpy /
 * DOLFINx types cross this boundary. All arrays are C-contiguous, cell-major ->
 * quadrature-point -> component ("AoS per point"), exactly the layout the reference hands to
 * and expects back from the user kernel (external_operator.py:286-290, 393-402).
 *
 * Conventions
 *   - every function returns 0 on success, <0 for an invalid argument (DXO_E_*), >0 for a
 *     HIP runtime error code (hipError_t). dxo_last_error(ctx) gives the text.
 *   - `mem` says where ALL data pointers of that call live: DXO_MEM_HOST (pageable or pinned
 *     host memory: the library does H2D -> kernel -> D2H, chunked and overlapped) or
 *     DXO_MEM_DEVICE (device memory on the ctx's GPU: the kernel is launched on the ctx
 *     stream and the call returns without synchronising).
 *   - the library never frees or keeps caller memory. Scratch is owned by the ctx.
 *   - non-convergence of a local Newton solve is NOT an error (the reference only reports
 *     niter / norm_res, demo_plasticity_mohr_coulomb.py:584-591).
 *   - one ctx per (process, device). Every entry point takes the ctx's mutex, so calls on one ctx
 *     from several host threads are serialised by the library (the reference calls from a single
 *     Python thread inside the SNES callback, petsc/petsc.py:60); use one ctx per thread for
 *     concurrency.
 */
#ifndef DXO_H
#define DXO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXO_ABI_VERSION 2

/* error codes (negative = caller error) */
#define DXO_OK 0
#define DXO_E_NULL (-1)      /* required pointer is NULL            */
#define DXO_E_DIM (-2)       /* unsupported tensor dimension d/gdim */
#define DXO_E_SIZE (-3)      /* negative size                       */
#define DXO_E_MEM (-4)       /* bad `mem` selector                  */
#define DXO_E_ALIGN (-5)     /* device pointer not 8-byte aligned   */
#define DXO_E_OPTION (-6)    /* unknown option / bad value          */
#define DXO_E_NODEVICE (-7)  /* no usable HIP device                */
#define DXO_E_SINGULAR (-8)  /* singular diagonal block (dxo_csr_block_jacobi) */

#define DXO_MEM_HOST 0
#define DXO_MEM_DEVICE 1

typedef struct dxo_ctx dxo_ctx;

/* Material constants of the von Mises demo (demo_plasticity_von_mises.py:185-188);
 * lmbda, mu, C_elas, deviatoric (:190-204) are derived from them inside the kernel. */
typedef struct dxo_vm_params {
    double E;        /* Young modulus            (70e3)               */
    double nu;       /* Poisson ratio            (0.3)                */
    double sigma_0;  /* yield strength           (250)                */
    double H;        /* hardening modulus        (E*Et/(E-Et), Et=E/100) */
} dxo_vm_params;

/* Constants of the Mohr-Coulomb demo (demo_plasticity_mohr_coulomb.py:110-116, 469). */
typedef struct dxo_mc_params {
    double E;        /* 6778                                          */
    double nu;       /* 0.25                                          */
    double c;        /* cohesion 3.45                                 */
    double phi;      /* friction angle  [rad]                         */
    double psi;      /* dilatancy angle [rad]                         */
    double theta_T;  /* Abbo-Sloan transition angle [rad]             */
    double a;        /* tension cut-off parameter 0.26 c / tan(phi)   */
    double tol;      /* relative residual tolerance 1e-8 (:469)       */
    int32_t nitermax;/* 200 (:469)                                    */
    int32_t _pad;
} dxo_mc_params;

/* Timing of the last call on a ctx, milliseconds (HIP events on the ctx streams). */
typedef struct dxo_timing {
    double h2d_ms;     /* DXO_MEM_HOST only, else 0                   */
    double kernel_ms;  /* sum over chunks                             */
    double d2h_ms;     /* DXO_MEM_HOST only, else 0                   */
    double total_ms;   /* first enqueue -> last completion            */
} dxo_timing;

typedef struct dxo_device_info {
    char name[128];
    char arch[32];          /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    int32_t compute_units;
    int32_t wavefront_size;
    int64_t total_mem_bytes;
} dxo_device_info;

/* ---- context ------------------------------------------------------------------------- */
int dxo_abi_version(void);
int dxo_device_count(int* count);
int dxo_ctx_create(int device, dxo_ctx** out);
int dxo_ctx_destroy(dxo_ctx* ctx);
const char* dxo_last_error(const dxo_ctx* ctx);
int dxo_ctx_device_info(dxo_ctx* ctx, dxo_device_info* info);
/* Borrow a caller-owned hipStream_t for DXO_MEM_DEVICE launches (NULL = library stream). */
int dxo_ctx_set_stream(dxo_ctx* ctx, void* hip_stream);
int dxo_ctx_synchronize(dxo_ctx* ctx);
/* Integer tuning knobs: "vm_variant" (0 scalar AoS kernel, 1 LDS-staged coalesced kernel,
 * default 1), "host_chunk_points" (points per H2D/kernel/D2H pipeline chunk),
 * "nontemporal" (0/1 streaming stores), "timing" (0/1 record dxo_timing on device calls),
 * "blocks_per_cu" (0 = one tile per wave — except that dxo_von_mises / dxo_vm_expand_tangent writing into a block from
 * dxo_vm_output_alloc use the launch shape its calibration found best; k = grid-stride over k workgroups per CU),
 * "mc_variant" (0 lane-per-point Newton; 1 classify kernel + compacted Newton kernel with lane refill; 2 — the default —
 * classification and Newton in one persistent kernel, plastic points queued per wave in LDS; outputs bit-identical),
 * "mc_blocks_per_cu" (variant 1: persistent Newton workgroups per CU, default 3), "mc_waves_per_simd" (variant 1),
 * "mc_part_points" (variant 1: points per classify/Newton pass, default and maximum 2^30: the compacted list holds int32
 * entries; variant 2 splits batches beyond 2^30 points by itself), "icnn_variant"
 * (fp32 network: 0 lane-per-point VALU kernel; 1 MFMA kernel on fp32-input MFMA; 2 — the default — the same GEMMs with
 * every fp32 operand split exactly into three bf16 numbers and six partial products on the bf16 MFMA pipe: fp32-level
 * results (it agrees with the oracle as closely as variant 1) in about 0.68 of the time; 3 and 4 — two kernels measured
 * slower in round 5 — exist only in a -DDXO_EXPERIMENTS build, scripts/exp/icnn_variants.h: this library answers them, like
 * "adjoint_patch" = 1, with DXO_E_OPTION), "host_small_bytes" (host batches whose inputs + outputs
 * fit this many bytes — default 8 MiB — and are not split by "host_chunk_points" take the SMALL path instead of the chunked
 * pipeline: the fixed cost per call at the reference's demo sizes; 0 switches the path off; per-phase dxo_timing is recorded
 * on it only with "timing" = 1, through one packed H2D and one packed D2H copy), "host_zero_copy_bytes" (default 8 MiB: on
 * that path, batches up to this size are not copied by DMA at all — the kernel reads and writes page-locked, device-mapped
 * HOST memory over PCIe directly: a caller's array that lies in a page-locked block this library handed out or registered
 * (dxo_host_alloc, dxo_host_register) is used IN PLACE, any other array goes through the context's pinned staging block (one
 * host memcpy each way); arrays that live on the device (dxo_vm_state) are used where they are; the batch runs in up to four
 * pieces of about "host_zero_copy_piece_bytes" (default 1 MiB, 0 = one piece), piece k + 1 being packed while piece k's kernel
 * runs. Results are bit-identical; 0 = off; with "timing" = 1 the copy form is used so that the phases can be timed; only the
 * operators whose kernels read every input once and store whole lines take this form — von Mises, heat, conductivity, Isihara
 * and their fused-operand forms; the Mohr-Coulomb and network kernels re-read inputs / store partial lines and keep the two
 * packed DMA copies. Measured (profiles/r06_demo_latency.txt): the von Mises demo's 15 000 points 194 -> 98 us per call),
 * "vm_host_tangent" (DXO_MEM_HOST dxo_von_mises: 0 = C_tang comes
 * back over PCIe, bit-identical to a device call; 1 = only (sigma, dp) cross PCIe and the caller's C_tang array is
 * rebuilt from them by the context's host threads while later chunks are in flight — same formulas as
 * dxo_vm_expand_tangent, agrees with the device tangent to rounding (5e-16 of its scale measured); the reference's 0/0
 *  point at f_el == 0 exactly is carried across in the sign bit of dp and comes out as NaN like in the copy mode),
 * "vm_mark_indeterminate" (default 0; 1 = DXO_MEM_DEVICE von Mises calls return dp = -0.0 — numerically 0 — at a point
 * with f_elastic == 0 EXACTLY, where the reference's n_elas is 0/0 and its tangent all NaN, demo_plasticity_von_mises.py:318,
 * so that dxo_vm_expand_tangent can reproduce that NaN from (sigma, dp); dxo_vm_clear_marks turns the marks back into +0;
 * the compact multi-GPU gathers set it themselves), "host_threads" (worker threads of that host half, default 32, capped by the CPUs the process may use: affinity mask and
 * cgroup CPU quota, minus two; DXO_HOST_CPU_BUDGET in the environment overrides the detection), "vm_rebuild_chunk_points" (pipeline chunk of that mode, default 2^17), "vm_rebuild_min_points" (default 2^16: smaller batches take the copy mode — back to back the rebuild wins from 15 000 points on, but calls that are milliseconds apart pay the wake-up of the host threads),
 * "wave_group_blocks" (the most workgroups of a persistent element kernel — operand evaluation, the fused field entries, the adjoint,
 * tangent, bilinear, hyperelastic and functional forms; 0, the default = "blocks_per_cu" of that kernel per compute unit; 1..65535,
 * rounded up to a multiple of 8; a wave walks the wave groups of its slice with the stride of the grid, so a small value sends every
 * wave round its loop several times on a small mesh; results do not depend on it; like "pmg_grid_blocks" it exists for tests),
 * and the "placement_*" options
 * of the output arena below. */
int dxo_ctx_set_option(dxo_ctx* ctx, const char* key, int64_t value);
int dxo_ctx_get_option(dxo_ctx* ctx, const char* key, int64_t* value);
int dxo_last_timing(dxo_ctx* ctx, dxo_timing* t);
/* Pinned host buffers (hipHostMalloc) so DXO_MEM_HOST calls DMA without staging. ctx may be NULL for both
 * (the memory belongs to the process; a buffer may outlive the context it was first used with). */
int dxo_host_alloc(dxo_ctx* ctx, int64_t bytes, void** ptr);
/* Page-lock / release memory the caller owns (hipHostRegister): e.g. the storage of the coefficient the results are
 * written into at every call (x.array of a fem.Function lives as long as the simulation). ctx may be NULL. */
int dxo_host_register(dxo_ctx* ctx, void* ptr, int64_t bytes);
int dxo_host_unregister(dxo_ctx* ctx, void* ptr);
int dxo_host_free(dxo_ctx* ctx, void* ptr);

/* ---- output arena: device memory for OUTPUT arrays, placed by calibration -------------------------------------
 * The kernels are HBM-bound and mostly stores (von Mises d = 6: 344 of 448 B per point). On MI355X the rate of a
 * multi-GB streaming-write sweep depends on the allocation it goes to (pure stores about 5.6-6.0, 6.4-6.5 or 6.9-7.1
 * TB/s; the class is stable for the life of the allocation and belongs to its virtual range, DESIGN.md 3.1,
 * profiles/r02_place_exp*.txt). dxo_output_alloc makes several ordinary allocations side by side, times one
 * streaming-write sweep on each, keeps the first above option "placement_good_GBps" (6800), else the fastest, and
 * frees the rest; the block is owned by the ctx (freed by dxo_output_free or dxo_ctx_destroy). Meant for the
 * persistent coefficient buffers a solver allocates once. Options: "placement_mode" 2 = hipMalloc candidates
 * (default), 0 = plain hipMalloc; "placement_candidates"
 * (default 16, at most 32, and never more than fit 60 % of the free memory together); "placement_min_bytes"
 * (default 1 GiB: smaller blocks are plain hipMalloc, a working set that small lives in the caches); "placement_vmm"
 * (default 1: three of every four candidates — 2: all of them — are virtual ranges backed by 2 MB physical chunks, hipMemCreate / hipMemMap,
 * which land in the fast class about twice as often as hipMalloc blocks and were the only fast ones for vm_tile on several boxes; 0 = hipMalloc candidates only, e.g. for buffers
 * that must be shareable through hipIpcGetMemHandle); "placement_probe" (default 1: candidates are ranked with a sweep in
 * the constitutive kernels' own pattern — three input streams read, three output streams written, 13 : 43 KiB per
 * 64-point tile, rates in algorithmic GB/s, early exit at "placement_good_mix_GBps" = 6250; 0: one stream of stores,
 * early exit at "placement_good_GBps"). A search can come up without a fast block: the winner is REJECTED — and one more search
 * with fresh candidates made while it stays allocated, the two winners then timed head to head — when it is below
 * "placement_accept_pct" (97) per cent of the best rate a calibration of this context ever kept for the same probe and
 * block size, or, without such a record, when it does not stand out from its own candidates (below
 * "placement_standout_pct" = 106 per cent of their median; once; not if it already runs at "placement_good_mix_GBps"); "placement_rounds" (3)
 * bounds the searches; the rate tested is the winner's rate AFTER the other candidates have been freed. The
 * calibration WRITES the block (zeros) and is synchronous. dxo_output_info reports what the calibration saw.
 * dxo_output_free RETAINS one calibrated block (the fastest it has been handed) instead of releasing it, and the next request of
 * exactly its size and probe is given that block back after a re-timing (rounds = 0 in its record: ~10 ms instead of a 2-7 s
 * search, and the only way to a fast block on a box where one range in 68 is fast); it is released when a search starts, when
 * dxo_device_alloc would otherwise fail, and with the context. Option "placement_cache" = 0 frees at once. */
#define DXO_PLACEMENT_MAX 32
typedef struct dxo_placement_info {
    int16_t mode;                           /* how the block was obtained: 0 plain hipMalloc, 2 candidates         */
    int16_t probe_kind;                     /* what the candidates were timed with: 0 one store stream, 1 the
                                               kernels' six-stream read + write sweep (option "placement_probe"),
                                               2 the von Mises kernel itself (dxo_vm_output_alloc), 3 the caller's
                                               launch (dxo_output_alloc_probed)                                     */
    int32_t candidates;                     /* ranges / allocations timed                                          */
    int32_t chosen;                         /* index of the one kept (-1: no calibration)                          */
    uint32_t vmm_mask;                      /* bit k: candidate k was built from 2 MB physical chunks (option
                                               "placement_vmm"), not by hipMalloc                                  */
    double probe_GBps[DXO_PLACEMENT_MAX];   /* streaming-write rate of each candidate                              */
    double calibration_ms;                  /* wall time of the whole call                                         */
    double chosen_GBps;                     /* rate of the block kept, re-timed after all but the three best
                                               candidates were freed (rates read low while many coexist)           */
    int32_t tuned_blocks_per_cu;            /* dxo_vm_output_alloc: launch shape of vm_tile that was fastest on the block
                                               kept (0 one tile per wave, k persistent workgroups per CU); the kernel
                                               uses it whenever it writes into this block and option "blocks_per_cu"
                                               is 0                                                                 */
    int32_t rounds;                         /* candidate searches this calibration made (1-3): a winner below 0.97 of the best
                                               rate the context ever kept for this probe and size, or one that does not stand
                                               out from its own candidates, buys one more search with fresh candidates      */
} dxo_placement_info;
int dxo_output_alloc(dxo_ctx* ctx, int64_t bytes, void** ptr);
int dxo_output_free(dxo_ctx* ctx, void* ptr);
int dxo_output_info(dxo_ctx* ctx, const void* ptr, dxo_placement_info* info);
/* The caller's own consumer as the probe. launch(block, shape, user) must enqueue ONE pass of the kernel that will write
 * the block — typically the dxo_* entry point itself with device pointers into `block` — on the context's launch stream
 * (dxo_ctx_set_stream, else the library's) and return without synchronising; it runs on the calling thread with the
 * context's (recursive) lock held. shapes: launch shapes to try (NULL / 0: one pass with shape 0); the best one is
 * recorded in tuned_blocks_per_cu for the caller to read back. bytes_per_launch: what a pass moves (for the GB/s of the
 * record; 0: the block size). probe_kind 3. */
typedef void (*dxo_probe_launch)(void* block, int shape, void* user);
int dxo_output_alloc_probed(dxo_ctx* ctx, int64_t bytes, dxo_probe_launch launch, void* user, double bytes_per_launch,
                            const int32_t* shapes, int n_shapes, void** ptr);
/* The output arrays of dxo_von_mises for n points of Mandel length d, as ONE arena block calibrated WITH THE KERNEL
 * ITSELF: every candidate is timed running vm_tile on synthetic inputs of the reference's distribution, in two launch
 * shapes (one tile per wave, 32 persistent workgroups per CU), and the block that makes the kernel fastest is kept
 * together with its shape (probe_kind 2). Generic sweeps rank blocks for ONE access pattern: blocks that topped a
 * store-stream or six-stream ranking ran the kernel anywhere between 5.3 and 6.4 TB/s (scripts/exp/archive/arena_eval.hip).
 * C_tang is the base of the block (pass it to dxo_output_free / dxo_output_info); sigma and dp start on 256-byte borders
 * behind it. Same options as dxo_output_alloc; blocks below "placement_min_bytes" are plain hipMalloc. */
int dxo_vm_output_alloc(dxo_ctx* ctx, int d, int64_t n, double** C_tang, double** sigma, double** dp);

/* ---- von Mises radial return + consistent tangent ---------------------------------------
 * Replaces return_mapping/_kernel + C_tang_impl, demo_plasticity_von_mises.py:298-352.
 *   d        Mandel vector length: 4 (plane strain, the reference demo) or 6 (3-D)
 *   n        number of quadrature points (num_cells * nq)
 *   deps     [n][d]   strain increment operand            (in)
 *   sigma_n  [n][d]   stress at the previous load step    (in; closure state, :347)
 *   p        [n]      cumulative plastic strain           (in; closure state, :348)
 *   C_tang   [n][d][d] consistent tangent                 (out; with DXO_MEM_DEVICE it may be NULL: only (sigma, dp)
 *                                                          are written, 160 instead of 448 B/point at d = 6, for callers
 *                                                          that rebuild the tangent with dxo_vm_expand_tangent)
 *   sigma    [n][d]   new stress                          (out)
 *   dp       [n]      plastic strain increment            (out)
 */
int dxo_von_mises(dxo_ctx* ctx, const dxo_vm_params* prm, int d, int64_t n, int mem,
                  const double* deps, const double* sigma_n, const double* p,
                  double* C_tang, double* sigma, double* dp);

/* Consistent tangent rebuilt from the RETURNED state: C_tang[n][d][d] from sigma[n][d], dp[n] (same formulas,
 * demo_plasticity_von_mises.py:318-324, with s = dev sigma). The multi-GPU gather exchanges (sigma, dp) and rebuilds
 * every tangent with this entry point. Agrees with dxo_von_mises' C_tang to rounding (<= 1e-14 of its scale; elastic points
 * bit for bit). A point whose dp is -0.0 (the producer's mark for the reference's 0/0 at f_elastic == 0, option
 * "vm_mark_indeterminate") comes out all NaN like the reference's tangent; without the mark such a point is C_elas. */
int dxo_vm_expand_tangent(dxo_ctx* ctx, const dxo_vm_params* prm, int d, int64_t n, int mem,
                          const double* sigma, const double* dp, double* C_tang);
/* dp[n] in DEVICE memory: every -0.0 (mark, see above) becomes +0.0, the value the reference holds there. Asynchronous on
 * the ctx stream. */
int dxo_vm_clear_marks(dxo_ctx* ctx, int64_t n, double* dp);

/* History update at the end of a load step, DEVICE memory only (demo_plasticity_von_mises.py:564-565):
 *   p[n] += dp[n];  sigma_n[n][d] = sigma[n][d].   One fused pass, asynchronous on the ctx stream. */
int dxo_vm_commit_state(dxo_ctx* ctx, int d, int64_t n, double* p, const double* dp,
                        double* sigma_n, const double* sigma);

/* ---- History variables resident on the device -------------------------------------------------
 * The reference's callback re-reads sigma_n and p from closure-captured host arrays at every call
 * (demo_plasticity_von_mises.py:347-348) although they change only at the end of a load step (:564-565). A dxo_vm_state
 * is their device mirror for n points of Mandel length d, plus the (sigma, dp) of the last call:
 *   dxo_vm_state_upload    host (or device) arrays -> mirror; blocking. Call it once, and again whenever the caller
 *                          changed its arrays in any other way than the load-step update below.
 *   dxo_von_mises_state    dxo_von_mises with sigma_n, p read from the mirror. `mem` says where deps and the outputs
 *                          live. DXO_MEM_HOST: only deps goes up (48 of 104 B/point at d = 6); option vm_host_tangent
 *                          applies as in dxo_von_mises. DXO_MEM_DEVICE: sigma / dp may be NULL (results stay in the
 *                          mirror, see dxo_vm_state_pointers).
 *   dxo_vm_state_commit    p += dp; sigma_n <- sigma inside the mirror with the results of the LAST call — what the
 *                          caller does to its host arrays at :564-565. Blocking. DXO_E_SIZE if there was no call since
 *                          the last upload / commit.
 *   dxo_vm_state_download  mirror -> caller's arrays (either may be NULL): checks and checkpoints.
 *   dxo_vm_state_pointers  the device arrays themselves: sigma_n[n][d], p[n], sigma[n][d], dp[n] (any may be NULL).
 * Results are bit-identical to dxo_von_mises on the same values. One state belongs to one ctx. */
typedef struct dxo_vm_state dxo_vm_state;
int dxo_vm_state_create(dxo_ctx* ctx, int d, int64_t n, dxo_vm_state** out);
void dxo_vm_state_destroy(dxo_ctx* ctx, dxo_vm_state* state);
int dxo_vm_state_upload(dxo_ctx* ctx, dxo_vm_state* state, int mem, const double* sigma_n, const double* p);
int dxo_vm_state_download(dxo_ctx* ctx, dxo_vm_state* state, int mem, double* sigma_n, double* p);
int dxo_vm_state_commit(dxo_ctx* ctx, dxo_vm_state* state);
int dxo_vm_state_pointers(dxo_ctx* ctx, dxo_vm_state* state, double** sigma_n, double** p, double** sigma, double** dp);
int dxo_von_mises_state(dxo_ctx* ctx, const dxo_vm_params* prm, dxo_vm_state* state, int mem, const double* deps,
                        double* C_tang, double* sigma, double* dp);

/* Device memory owned by the caller but allocated through the library (hipMalloc / hipFree / hipMemcpyAsync on
 * the ctx stream + synchronise), so a host program without its own HIP binding can keep state on the GPU.
 * kind: 0 host->device, 1 device->host, 2 device->device. */
int dxo_device_alloc(dxo_ctx* ctx, int64_t bytes, void** ptr);
int dxo_device_free(dxo_ctx* ctx, void* ptr);
int dxo_copy(dxo_ctx* ctx, void* dst, const void* src, int64_t bytes, int kind);

/* ---- nonlinear heat flux ------------------------------------------------------------------
 * Replaces k / q_impl / dqdT_impl / dqdsigma_impl, demo_nonlinear_heat_equation_part2.py:209-261
 * (same code: test/test_external_operators_evaluation.py:64-86).
 *   T [n], sigma [n][gdim] (in);  q [n][gdim], dqdT [n][gdim], dqdsigma [n][gdim][gdim] (out).
 * Any output may be NULL (the reference evaluates the three derivatives as separate
 * operators; one fused launch fills whichever are requested). gdim in {1,2,3}.
 */
int dxo_heat(dxo_ctx* ctx, double A, double B, int gdim, int64_t n, int mem,
             const double* T, const double* sigma,
             double* q, double* dqdT, double* dqdsigma);

/* Scalar conductivity of the part-1 heat demo: k[n] = 1 / (A + B T[n]) and dkdT[n] = -B k^2 (k_impl / dkdT_impl,
 * demo_nonlinear_heat_equation_part1.py:251-271). Either output may be NULL; one fused pass. The operator lives on a CG
 * space in the demo: its values reach the coefficient through the dofmap assigner (dxo_assign below). */
int dxo_conductivity(dxo_ctx* ctx, double A, double B, int64_t n, int mem, const double* T, double* k, double* dkdT);

/* ---- Mohr-Coulomb (Abbo-Sloan) return mapping + AD-through-Newton tangent ----------------------
 * Replaces return_mapping / dsigma_ddeps_vec / C_tang_impl,
 * demo_plasticity_mohr_coulomb.py:282-391, 405-462, 469-533, 555, 574-593.
 *   deps [n][4], sigma_n [n][4] (in; sigma_n is closure state, :579);
 *   C_tang [n][4][4] = d sigma / d deps differentiated THROUGH the Newton iterations (jacfwd of the
 *   while_loop, :555), sigma [n][4] (out).
 *   optional diagnostics (NULL to skip) = the reference's aux outputs (:533, :582):
 *   niter [n] int32, yielding [n] = f(sigma_n + C deps), norm_res [n], dlambda [n].
 * A point that does not converge within prm->nitermax iterations is not an error: niter == nitermax
 * and norm_res tell (the reference prints the same, :584-591).
 * DXO_MEM_DEVICE needs 16-byte aligned deps/sigma_n/C_tang/sigma. */
int dxo_mohr_coulomb(dxo_ctx* ctx, const dxo_mc_params* prm, int64_t n, int mem,
                     const double* deps, const double* sigma_n,
                     double* C_tang, double* sigma,
                     int32_t* niter, double* yielding, double* norm_res, double* dlambda);

/* The same model for a six-component strain, the full 3-D form of dxo_mohr_coulomb: Mandel order
 * (xx, yy, zz, sqrt2 xy, sqrt2 xz, sqrt2 yz), the order of the `eps` operand of a gdim = 3 mesh.
 *   deps [n][6], sigma_n [n][6] (in);  C_tang [n][6][6] = d sigma / d deps through the Newton iterations, sigma [n][6] (out);
 *   the same dxo_mc_params, the same optional diagnostics (dxo_mc_summary works on them), the same checks and error codes.
 * The surface is a function of I1, J2 = s:s / 2 and J3 = det s; with zero out-of-plane shears in deps and sigma_n the in-plane
 * entries are dxo_mohr_coulomb's. C_tang is the [n][6][6] block of the ("eps", "eps", bs = 3) bilinear pair and of
 * tangent_apply, sigma the operand of the internal force. Kernels: classification (elastic points finished at HBM speed) +
 * compacted Newton with lane refill; ctx option "mc_variant" = 0 selects the plain lane-per-point kernel (bit-identical),
 * "mc_part_points" the points per classify / Newton pass. DXO_MEM_DEVICE needs 16-byte aligned deps/sigma_n/C_tang/sigma. */
int dxo_mohr_coulomb3(dxo_ctx* ctx, const dxo_mc_params* prm, int64_t n, int mem,
                      const double* deps, const double* sigma_n,
                      double* C_tang, double* sigma,
                      int32_t* niter, double* yielding, double* norm_res, double* dlambda);

/* History variable resident on the device, the Mohr-Coulomb counterpart of dxo_vm_state: the
 * reference's callback re-reads sigma_n from a closure-captured host array at every call
 * (demo_plasticity_mohr_coulomb.py:579) although it changes only at the end of a load step
 * (:728, `sigma_n.x.array[:] = sigma.ref_coefficient.x.array`). A dxo_mc_state mirrors sigma_n[n][4] and keeps the
 * stress of the last call:
 *   dxo_mc_state_upload     caller's array -> mirror; blocking. Once, and again after any change other than the commit.
 *   dxo_mohr_coulomb_state  dxo_mohr_coulomb with sigma_n read from the mirror; `mem` says where deps and the outputs live
 *                           (DXO_MEM_HOST: only deps goes up, 32 of 64 B/point; DXO_MEM_DEVICE: sigma may be NULL, the
 *                           result stays in the mirror, see dxo_mc_state_pointers).
 *   dxo_mc_state_commit     sigma_n <- sigma of the LAST call inside the mirror (:728). Blocking. DXO_E_SIZE if there was
 *                           no call since the last upload / commit; a state of n = 0 points commits trivially.
 *   dxo_mc_state_download   mirror -> caller's array (checks, checkpoints);  dxo_mc_state_pointers: the device arrays.
 * Results are bit-identical to dxo_mohr_coulomb on the same values. One state belongs to one ctx. */
typedef struct dxo_mc_state dxo_mc_state;
int dxo_mc_state_create(dxo_ctx* ctx, int64_t n, dxo_mc_state** out);
void dxo_mc_state_destroy(dxo_ctx* ctx, dxo_mc_state* state);
int dxo_mc_state_upload(dxo_ctx* ctx, dxo_mc_state* state, int mem, const double* sigma_n);
int dxo_mc_state_download(dxo_ctx* ctx, dxo_mc_state* state, int mem, double* sigma_n);
int dxo_mc_state_commit(dxo_ctx* ctx, dxo_mc_state* state);
int dxo_mc_state_pointers(dxo_ctx* ctx, dxo_mc_state* state, double** sigma_n, double** sigma);
int dxo_mohr_coulomb_state(dxo_ctx* ctx, const dxo_mc_params* prm, dxo_mc_state* state, int mem, const double* deps,
                           double* C_tang, double* sigma, int32_t* niter, double* yielding, double* norm_res,
                           double* dlambda);

/* Inner-Newton summary of a dxo_mohr_coulomb call whose diagnostics live in DEVICE memory: the numbers the
 * reference prints at every call (unique iteration counts and their multiplicities, max f, max residual,
 * demo_plasticity_mohr_coulomb.py:584-591), reduced on the GPU (wave __shfl_xor maxima, LDS histogram).
 *   niter [n] int32 (device); yielding / norm_res [n] (device, may be NULL)
 *   hist [nbins] (host, out): hist[k] = #points with niter == k (k >= nbins-1 clamps into the last bin);
 *   nbins <= 1024, use prm->nitermax + 1.   max_* (host, out, may be NULL): maxima over non-NaN entries,
 *   -inf if none; nan_counts[2] (host, out, may be NULL): NaN entries of yielding / norm_res. Blocking. */
int dxo_mc_summary(dxo_ctx* ctx, int64_t n, const int32_t* niter, const double* yielding, const double* norm_res,
                   int nbins, int64_t* hist, double* max_yielding, double* max_norm_res, int64_t* nan_counts);

/* ---- ICNN hyperelastic surrogate: stress P = dW/dF and tangent dP/dF --------------------------
 * Replaces ICNN.forward + compute_stress_local + vmap(jacfwd(.)) + dP_dF_impl,
 * demo_hyperelasticity.py:256-300, 362-381, 429-456. The weight struct takes the tensors of the
 * reference's state_dict as they are stored (fp32, row-major [out][in]); softplus on the convex
 * layers (:238) and the fold of the activation-free layer 0 into layer 1 happen inside create().
 * Architecture is the demo's: n_input 3, n_hidden [64, 64, 64], n_output 1 (:302-307).
 *   F  [n][4] = (F11, F12, F21, F22) (in);  dP [n][4][4] with dP[i][j] = dP_i/dF_j, P [n][4] (out),
 *   the reference's return order is (dP, P) (:456).
 *   precision 0: network in fp32 like the reference (`.float()`, :286); 1: network in fp64
 *   (BASELINE config 5's fp64-vs-fp32 tolerance study). Features and chain rule are fp64 in both. */
typedef struct dxo_icnn_weights {
    const float* layers0_weight;   /* layers.0.weight        [64][3]  */
    const float* layers0_bias;     /* layers.0.bias          [64]     */
    const float* layers1_weights;  /* layers.1.weights       [64][64] */
    const float* skip1_weight;     /* skip_layers.1.weight   [64][3]  */
    const float* skip1_bias;       /* skip_layers.1.bias     [64]     */
    const float* layers2_weights;  /* layers.2.weights       [64][64] */
    const float* skip2_weight;     /* skip_layers.2.weight   [64][3]  */
    const float* skip2_bias;       /* skip_layers.2.bias     [64]     */
    const float* layers3_weights;  /* layers.3.weights       [1][64]  */
    const float* skip3_weights;    /* skip_layers.3.weights  [1][3]   */
    int32_t n_hidden;              /* 64                               */
    int32_t _pad;
} dxo_icnn_weights;
typedef struct dxo_icnn dxo_icnn;
int dxo_icnn_create(dxo_ctx* ctx, const dxo_icnn_weights* w, dxo_icnn** out);
int dxo_icnn_destroy(dxo_ctx* ctx, dxo_icnn* model);
/* H_flat[4] of the stress correction P_cor = F @ H (:371), computed by create() at F = I. */
int dxo_icnn_correction(dxo_ctx* ctx, const dxo_icnn* model, double* H_flat);
int dxo_icnn_eval(dxo_ctx* ctx, const dxo_icnn* model, int precision, int64_t n, int mem,
                  const double* F, double* dP, double* P);

/* Analytic Isihara energy the network was trained on (demo_hyperelasticity.py:686-703; UFL-only in the reference):
 *   W = c1 (I1bar-3) + c2 (I2bar-3) + c3 (I1bar-3)^2 + c4 (J-1)^2,  reference constants (0.5, 1.0, 1.0, 1.5).
 * Same I/O as dxo_icnn_eval: F[n][4] -> dP[n][4][4] (dP_i/dF_j), P[n][4], fp64 throughout. det F <= 0 -> NaN. */
typedef struct dxo_isihara_params { double c1, c2, c3, c4; } dxo_isihara_params;
int dxo_isihara(dxo_ctx* ctx, const dxo_isihara_params* prm, int64_t n, int mem,
                const double* F, double* dP, double* P);

/* ---- operand evaluation on the device ----------------------------------------
 * Device counterpart of `fem.Expression(operand, points).eval(mesh, entities)` as evaluate_operands calls it
 * (src/dolfinx_external_operator/external_operator.py:386-402) for operands that are linear in the value or the
 * gradient of ONE Lagrange field (every operand of the reference's demos). The mesh/element description is
 * uploaded once (dxo_mesh_create); each call gathers the field's dofs and writes (n_cells, nq, value_size)
 * doubles in Expression.eval's C order.
 *   dofmap       = V.dofmap.list            [num_cells][ndofs]  node indices (unblocked); field vector u is
 *                                            blocked: u[node*bs + i], as fem.Function.x.array
 *   geom_dofmap  = mesh.geometry.dofmap     [num_cells][ngeom]
 *   x            = mesh.geometry.x          [num_geom_nodes][x_stride]  (DOLFINx: x_stride = 3), first gdim used
 *   phi, dphi    = V.element.basix_element.tabulate(1, points): values [nq][ndofs], reference gradients
 *                  [nq][ndofs][gdim]; dpsi = the coordinate element's reference gradients [nq][ngeom][gdim]
 * Cells are not assumed affine: J is rebuilt at every point from dpsi.
 * Block sizes: value / grad / value_grad act on each component alone and take ANY bs in 1..DXO_OPERAND_MAX_BS (the reference hands
 * `fem.Expression` whatever field the operand is: test/test_nested_ex_op.py:113-118 evaluates a 4-component DG field): bs = 1 and bs = gdim run
 * the dense kernels, any other bs one scalar launch per component. The kinds built from grad u of a displacement-like field need bs = gdim.
 * The adjoint entry points take bs = 1 or gdim. */
#define DXO_OPERAND_MAX_BS 64
enum {
    DXO_OPERAND_VALUE = 0,       /* u                       value_size = bs                         (heat: T)        */
    DXO_OPERAND_GRAD = 1,        /* grad u, [i][j]=du_i/dx_j value_size = bs*gdim                    (heat: grad T)   */
    DXO_OPERAND_EPS_MANDEL = 2,  /* [g00,g11,0,r(g01+g10)] (2-D, demo_plasticity_von_mises.py:225-227),
                                    [g00,g11,g22,r(g01+g10),r(g02+g20),r(g12+g21)] (3-D), r = sqrt(2)/2; bs = gdim   */
    DXO_OPERAND_DEFGRAD = 3,     /* I + grad u, row-major   value_size = gdim*gdim (demo_hyperelasticity.py:479)      */
    DXO_OPERAND_VALUE_GRAD = 4,  /* [u (bs), grad u (bs*gdim)] in one pass, value_size = bs*(1+gdim) (heat: T and grad T)   */
    /* NONLINEAR operands of one vector field (bs = gdim), formed per point from F = I + grad u — the operand of the reference's own
     * operand test, test/test_operands_evaluation.py:32-36 (F = Identity(d) + grad(u); C = F.T * F; J = det(F); I1 = tr(C)).
     * Forward evaluation only (dxo_eval_operand, dxo_eval_operand_facets): dxo_operand_adjoint answers DXO_E_OPTION for them
     * (the adjoint of a nonlinear operand is a linearisation, which UFL derives on the reference side). */
    DXO_OPERAND_CAUCHY_GREEN = 5,/* C = F^T F, row-major     value_size = gdim*gdim                                          */
    DXO_OPERAND_I1 = 6,          /* tr(F^T F) = sum F_ij^2   value_size = 1                                                  */
    DXO_OPERAND_DETF = 7,        /* det F                    value_size = 1                                                  */
    DXO_OPERAND_DIV = 8          /* div u = tr(grad u)       value_size = 1, bs = gdim; LINEAR: forward and adjoint
                                    (the operand of test/test_external_operators_evaluation.py:141)                           */
};
typedef struct dxo_mesh_desc {
    int32_t gdim;               /* 2 or 3 (= topological dimension) */
    int32_t nq;                 /* quadrature points per cell, <= 64 */
    int32_t ndofs;              /* scalar basis functions per cell of the field's element */
    int32_t ngeom;              /* basis functions per cell of the coordinate element */
    int32_t x_stride;           /* doubles per node in x (0 = gdim) */
    int32_t _pad;
    int64_t num_cells, num_field_nodes, num_geom_nodes;
    const double* phi;
    const double* dphi;
    const double* dpsi;
    const int32_t* dofmap;
    const int32_t* geom_dofmap;
    const double* x;
} dxo_mesh_desc;
typedef struct dxo_mesh dxo_mesh;
int dxo_mesh_create(dxo_ctx* ctx, const dxo_mesh_desc* desc, dxo_mesh** out);   /* host pointers; copies everything */
int dxo_mesh_destroy(dxo_ctx* ctx, dxo_mesh* mesh);
/* value_size of an operand, or a negative error code if (gdim, bs, kind) is unsupported */
int dxo_operand_value_size(int gdim, int bs, int kind);
/* u: field vector (num_field_nodes*bs doubles); cells: entity list or NULL for cells [0, n_cells) (n_cells < 0: all);
 * out: n_cells*nq*value_size doubles. mem applies to u, cells and out alike. */
/* The operand `x = ufl.SpatialCoordinate(mesh)` (test/test_nested_ex_op.py:113-118): the physical position of every quadrature point,
 * x(xi_q) = sum_v psi_v(xi_q) X_v with the coordinate element's own basis. psi = its VALUES at the quadrature points, [nq][ngeom] (the mesh
 * description carries the gradients only), given once; out: n_cells*nq*gdim doubles, cells / n_cells / mem as for dxo_eval_operand. */
int dxo_mesh_set_coordinate_values(dxo_ctx* ctx, dxo_mesh* mesh, const double* psi);
int dxo_eval_coordinate(dxo_ctx* ctx, dxo_mesh* mesh, int mem, const int32_t* cells, int64_t n_cells, double* out);
int dxo_eval_operand(dxo_ctx* ctx, dxo_mesh* mesh, int kind, int bs, int mem, const double* u,
                     const int32_t* cells, int64_t n_cells, double* out);

/* Codim-1 entities. evaluate_operands hands its `entities` to Expression.eval unchanged (external_operator.py:340, 402);
 * for an operator on a facet sub-mesh they are (cell, local_facet) pairs (test/test_codim_external_operator.py:76-84, 111)
 * and the points are quadrature points of the reference FACET mapped into the reference cell per local facet.
 * dxo_mesh_set_facet_tables uploads the tables tabulated at those mapped points, one set per local facet:
 *   phi [n_local_facets][nq][ndofs], dphi [n_local_facets][nq][ndofs][gdim], dpsi [n_local_facets][nq][ngeom][gdim]
 * (host pointers). dxo_eval_operand_facets: entities [n_entities][2] int32 = (cell, local facet); out
 * [n_entities][nq][value_size]; the gradient is the full physical gradient at the facet points. mem applies to u,
 * entities and out alike; with DXO_MEM_DEVICE the entity list is not range-checked. */
int dxo_mesh_set_facet_tables(dxo_ctx* ctx, dxo_mesh* mesh, int n_local_facets, int nq, const double* phi,
                              const double* dphi, const double* dpsi);
int dxo_eval_operand_facets(dxo_ctx* ctx, dxo_mesh* mesh, int kind, int bs, int mem, const double* u,
                            const int32_t* entities, int64_t n_entities, double* out);

/* Operand evaluation FUSED in front of the von Mises return map: one launch for the demo's
 * evaluate_operands + evaluate_external_operators pair (demo_plasticity_von_mises.py:445-456) when the operand is
 * eps(u) of a vector Lagrange field on `mesh` (gdim 2 -> d = 4, gdim 3 -> d = 6). u: num_field_nodes*gdim doubles;
 * state and outputs cover ALL cells of the mesh in cell order: n = num_cells*nq points, same layout and meaning as
 * dxo_von_mises. The strain increment is never written to memory. With DXO_MEM_DEVICE C_tang may be NULL: (sigma, dp) only, for a
 * matrix-free solve that forms the tangent's action from them (dxo_tangent_apply_vm below). */
int dxo_von_mises_field(dxo_ctx* ctx, const dxo_vm_params* prm, dxo_mesh* mesh, int mem, const double* u,
                        const double* sigma_n, const double* p, double* C_tang, double* sigma, double* dp);
/* The same with the history variables in a dxo_vm_state (n = num_cells*nq, d as the mesh gives it): a host call sends the
 * dof vector only. Option vm_host_tangent applies to both entry points (DXO_MEM_HOST). */
int dxo_von_mises_field_state(dxo_ctx* ctx, const dxo_vm_params* prm, dxo_mesh* mesh, dxo_vm_state* state, int mem,
                              const double* u, double* C_tang, double* sigma, double* dp);

/* ---- the consumer side on the device, DEVICE memory only ---------------------------------
 * In the reference the coefficient is consumed by DOLFINx assembly of inner(sigma, eps(v)) dx and of the Jacobian
 * form `_apply_derivative_tensor` builds (src/dolfinx_external_operator/external_operator.py:463-486;
 * demo_plasticity_von_mises.py:378-391). These two entry points are the ADJOINT of dxo_eval_operand, so a
 * matrix-free Newton-Krylov solver can leave sigma and C_tang in HBM and move only dof vectors:
 *   dxo_operand_adjoint : out[dof] += sum_q w_q |det J_q| B_q^T s_q   for a quadrature field s of the operand's shape
 *                         (kind EPS_MANDEL with s = sigma: the internal force; GRAD with s = q: the heat residual)
 *   dxo_tangent_apply   : out[dof] += sum_q w_q |det J_q| B_q^T C_tang_q B_q v   (eps / Mandel, bs = gdim), K never formed
 * `out` is ACCUMULATED into (zero it first) — unless option "consumer_overwrite" = 1, with which these calls (and
 * dxo_tangent_*_vm, dxo_tangent_diagonal, dxo_von_mises_residual) SET out to the assembled vector: a Krylov matvec then needs no
 * memset and the node sums no read of out. S / C_tang are laid out like the operator outputs, (n_cells, nq, ...).
 * Full-mesh calls write element vectors and add them per node in the fixed order of the transposed dofmap (no atomics,
 * bit-reproducible); entity subsets, or option "adjoint_atomics" = 1, add with fp64 hardware atomics instead
 * (reproducible to rounding only). Option "adjoint_cell" = 0 switches off the lane-per-cell kernel that the internal
 * force (kind EPS_MANDEL) uses on the standard elements. On hexahedra with the 2x2x2 rule (8 or 27 nodes) the element vectors
 * f_a = sum_q dphi_a(xi_q) . T_q of a wave's 8 cells are formed on the fp64 matrix pipe, [32 x 24] x [24 x 24] as 24
 * v_mfma_f64_16x16x4_f64 (option "adjoint_mfma", default 1; 0 = the round-4 DPP reduce-scatter over a cell's 8 lanes; both are
 * bit-reproducible, they differ from each other in the last bits: a different order of the 8-point sum). The state-based forms
 * (dxo_tangent_apply_vm, dxo_tangent_diagonal_vm) do the same on P2 triangles with the 3-point rule and P2 tetrahedra with the
 * 4-point rule (6 / 9 instructions per wave group; 0 = the lane = (cell, node) loop over tensors parked in LDS).
 * C_tang of dxo_tangent_apply / dxo_tangent_diagonal must be 16-byte aligned (the operator kernels' outputs are).
 * dxo_mesh_set_weights: the nq reference quadrature weights (basix.make_quadrature(...)[1]), host pointer. */
int dxo_mesh_set_weights(dxo_ctx* ctx, dxo_mesh* mesh, const double* weights);
int dxo_operand_adjoint(dxo_ctx* ctx, dxo_mesh* mesh, int kind, int bs, const double* S, const int32_t* cells,
                        int64_t n_cells, double* out);
int dxo_tangent_apply(dxo_ctx* ctx, dxo_mesh* mesh, const double* C_tang, const double* v, double* out);
/* The same two operators for the von Mises operator WITHOUT its tangent array (round 4): the consistent tangent is a function of the
 * returned state (dxo_vm_expand_tangent), so K v and diag(K) are formed from (sigma, dp) — 56 instead of 288 bytes per point at
 * d = 6, ~40 flops per point instead of 36 loads and FMAs. A matrix-free Newton-Krylov solve then never needs C_tang to exist:
 * dxo_von_mises_field / _field_state accept C_tang = NULL on the device path (160 instead of 448 bytes per point) and every Krylov
 * matvec reads a fifth of the bytes. sigma [n][d] (16-byte aligned), dp [n]: the operator's outputs for all cells of the mesh in cell
 * order (e.g. the arrays of dxo_vm_state_pointers); prm: the parameters the operator ran with. Agrees with dxo_tangent_apply on the
 * C_tang of the same call to rounding (1e-13 of the scale; a point the producer marked with dp = -0.0 gives the reference's NaN). */
int dxo_tangent_apply_vm(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_vm_params* prm, const double* sigma, const double* dp,
                         const double* v, double* out);
int dxo_tangent_diagonal_vm(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_vm_params* prm, const double* sigma, const double* dp, double* out);
/* The residual evaluation of a von Mises Newton iteration in ONE call (DEVICE pointers; demo_plasticity_von_mises.py:445-456 followed
 * by the assembly of inner(sigma, eps(v)) dx, :266): (sigma, dp) = return map of (eps(u), sigma_n, p) exactly as dxo_von_mises_field
 * returns them with C_tang = NULL, and R[dof] += sum_q w|J| B^T sigma as dxo_operand_adjoint(EPS_MANDEL) adds it: the two launches back to
 * back on the context's stream. Option "vm_residual_fused" = 1 selects, on Q2 hexahedra with the 2x2x2 rule, ONE kernel that scatters the
 * stress from the registers it was returned in (round 5, with the scatter on the matrix pipe: 1.11 against 1.14-1.16 ms per 10^7 points;
 * R then differs from the two launches' in the last bits — another order of the Jacobian's sums — hence off by default). sigma_n, sigma 16-byte aligned. */
int dxo_von_mises_residual(dxo_ctx* ctx, const dxo_vm_params* prm, dxo_mesh* mesh, const double* u, const double* sigma_n,
                           const double* p, double* sigma, double* dp, double* R);
/* out[dof] += K_(dof,dof): the diagonal of the same operator (Jacobi preconditioner of a matrix-free Krylov solve). */
int dxo_tangent_diagonal(dxo_ctx* ctx, dxo_mesh* mesh, const double* C_tang, double* out);
/* The bilinear form of a general PAIR of linear operand kinds of one field with block size bs, per-point block C (DEVICE pointers):
 *   dxo_bilinear_apply    : out[dof] += sum_q w_q |det J_q| B_test,q^T C_q B_trial,q v
 *   dxo_bilinear_diagonal : out[dof] += sum_q w_q |det J_q| (B_test,q^T C_q B_trial,q)_(dof,dof)
 * C: [n][D_test][D_trial] row-major fp64, n = num_cells*nq points of ALL cells of the mesh in cell order (no entity subsets), D_* the
 * value size of the kind (dxo_operand_value_size); 16-byte aligned, as the operator outputs are. Supported pairs (test, trial):
 *   bs = gdim : (GRAD | DEFGRAD, GRAD | DEFGRAD)  finite strain, C = dP/dF of dxo_isihara[_field] / dxo_icnn[_field] ([n][4][4] in 2-D);
 *                                                 DEFGRAD stands for its linearisation, grad
 *               (EPS_MANDEL, EPS_MANDEL)          agrees with dxo_tangent_apply / dxo_tangent_diagonal on the same C_tang
 *   bs = 1    : (GRAD, VALUE_GRAD)                heat: C = [dq/dT | dq/dsigma], [n][gdim][1 + gdim]
 *               (GRAD, GRAD), (VALUE, VALUE), (VALUE_GRAD, VALUE_GRAD)
 * Any other pair, and the nonlinear kinds (C, I1, det F), return DXO_E_OPTION with a message in dxo_last_error. The quadrature weights
 * must be set (dxo_mesh_set_weights; DXO_E_OPTION otherwise). `out` is accumulated into, or SET with option "consumer_overwrite" = 1;
 * option "adjoint_atomics" as for dxo_tangent_apply (default: element vectors + node sums, bit-reproducible). The first call on a mesh
 * allocates the element-vector buffer; later calls allocate nothing (capture-safe).
 *   dxo_bilinear_apply_t  : out[dof] += sum_q w_q |det J_q| B_trial,q^T C_q^T B_test,q v, the action of the TRANSPOSED operator (adjoint
 * solves). (test_kind, trial_kind), the C array and its layout [n][D_test][D_trial] are those of the forward call: the caller
 * transposes nothing, the kernel reads t = C^T e from the same staged block. The pair table, the DEFGRAD rule, the checks and the
 * options "consumer_overwrite" and "adjoint_atomics" are those of dxo_bilinear_apply; two-pass scatter, bit-reproducible. The diagonal
 * of the transpose is the diagonal: dxo_bilinear_diagonal serves both. */
int dxo_bilinear_apply(dxo_ctx* ctx, dxo_mesh* mesh, int test_kind, int trial_kind, int bs, const double* C, const double* v, double* out);
int dxo_bilinear_diagonal(dxo_ctx* ctx, dxo_mesh* mesh, int test_kind, int trial_kind, int bs, const double* C, double* out);
int dxo_bilinear_apply_t(dxo_ctx* ctx, dxo_mesh* mesh, int test_kind, int trial_kind, int bs, const double* C, const double* v, double* out);
/* The same bilinear form ASSEMBLED into a sparse matrix on the device: what the demos hand to their LU solve,
 * assemble_matrix(J_replaced, bcs) (demo_plasticity_von_mises.py:422-434, demo_plasticity_mohr_coulomb.py:662-675,
 * demo_hyperelasticity.py:560-573; the heat demo compares assembled matrices, demo_nonlinear_heat_equation_part2.py:313-335).
 * dxo_csr_create  : the CSR pattern of one Lagrange field with block size bs (1 or gdim) on `mesh`, built once on the host from the
 *                   mesh's dofmap. Rows and columns are the blocked dofs node*bs + i (DOLFINx's numbering of a serial blocked space);
 *                   row r holds every column whose node shares a cell with r's node, for all bs components, sorted ascending; the
 *                   diagonal is always present. row_ptr is int64 [n_rows + 1], col int32 [nnz] (2^31 dofs or more: DXO_E_SIZE).
 * dxo_csr_info    : sizes, the DEVICE arrays owned by the pattern, and the pattern's build time in ms; any pointer may be NULL.
 * dxo_bilinear_assemble : values[nnz] += sum_cells sum_q w_q |det J_q| B_test,q^T C_q B_trial,q, for the pairs and the C layout of
 *                   dxo_bilinear_apply (DEVICE pointers; all cells of the mesh). DXO_E_OPTION for other pairs or missing weights,
 *                   DXO_E_DIM for a pattern of another mesh or block size. Option "consumer_overwrite" = 1 SETs values. Default form:
 *                   element matrices of a chunk of cells (option "assemble_chunk_cells", 0 = as many as fit 1 GiB of scratch) go to a
 *                   scratch buffer, then one thread per row adds them in ascending cell order: atomic-free, bit-reproducible and
 *                   bitwise independent of the chunk size. Option "adjoint_atomics" = 1: fp64 atomics into values (reproducible to
 *                   rounding only). The first call on a pattern allocates the scratch; later calls allocate nothing (capture-safe).
 * dxo_csr_dirichlet : the rows and columns of the constrained dofs (DEVICE int32 list; out-of-range entries are ignored) are zeroed
 *                   and their diagonal entries set to `diagonal`, as assemble_matrix(a, bcs, diagonal) does (one thread per row,
 *                   deterministic, capture-safe). */
typedef struct dxo_csr dxo_csr;
int dxo_csr_create(dxo_ctx* ctx, dxo_mesh* mesh, int bs, dxo_csr** out);
int dxo_csr_destroy(dxo_ctx* ctx, dxo_csr* csr);
int dxo_csr_info(dxo_ctx* ctx, const dxo_csr* csr, int64_t* n_rows, int64_t* nnz, const int64_t** row_ptr, const int32_t** col,
                 double* build_ms);
int dxo_bilinear_assemble(dxo_ctx* ctx, dxo_mesh* mesh, dxo_csr* csr, int test_kind, int trial_kind, int bs, const double* C,
                          double* values);
int dxo_csr_dirichlet(dxo_ctx* ctx, dxo_csr* csr, const int32_t* dofs, int64_t n_dofs, double diagonal, double* values);

/* ---- linear solves on the device (csrc/krylov.hip), DEVICE memory only ----------------------------------------
 * dxo_csr_spmv    : y = alpha A x + beta y for the matrix `values` on a dxo_csr pattern (BLAS semantics: with beta == 0, y is not
 *                   read). A group of lanes owns one node and forms all bs rows of it, reading one column index per neighbouring node;
 *                   no atomics, bit-reproducible. Option "spmv_lanes": lanes per node (8, 16, 32, 64; default 0 = from the mean
 *                   neighbour count). Capture-safe.
 * dxo_csr_transpose : values_t[(n,i),(m,j)] = values[(m,j),(n,i)] on the SAME pattern (csrc/transpose.hip): the pattern of
 *                   dxo_csr_create is structurally symmetric, so the transposed matrix keeps the row pointers, columns, Dirichlet mask,
 *                   block-Jacobi layout and multigrid symbolic phase, and only the values are permuted. Pure data movement: exact.
 *                   values_t == values transposes in place (each off-diagonal block pair is exchanged by the one thread that owns the
 *                   smaller node, a diagonal block is transposed by its own thread); any other overlap is the caller's error. One
 *                   grid-stride kernel, deterministic. dxo_csr_dirichlet commutes with it (rows and columns are both zeroed).
 * dxo_csr_spmv_t  : y = alpha A^T x + beta y without forming A^T (BLAS semantics: with beta == 0, y is not read), in the lane-group
 *                   shape and with the option "spmv_lanes" of dxo_csr_spmv: a lane reads the mirrored block of each of its neighbour
 *                   blocks in the rows of the neighbour and performs the fused multiply-adds of dxo_csr_spmv on the transposed values
 *                   in the same order, so the result equals dxo_csr_spmv of dxo_csr_transpose's output bit for bit. No atomics.
 *                   Both calls share the MIRROR MAP of the pattern (for block k of node n, the position of n among the blocks of the
 *                   column node's row; uint16 per block), built on the device at the first of these calls on a pattern and kept in
 *                   the dxo_csr: that first call allocates and synchronises once, later calls allocate and synchronise nothing
 *                   (capture-safe). Patterns of dxo_csr_create (bs 1, 2, 3) only: a pattern without a mesh (a multigrid level)
 *                   answers DXO_E_DIM, a pattern found not structurally symmetric DXO_E_OPTION with a message; NULL and alignment
 *                   errors as dxo_csr_spmv.
 * dxo_csr_block_jacobi : inv[n_rows/bs][bs][bs] = the inverses of the bs x bs diagonal blocks (closed form, bs <= 3; bs = 1 is point
 *                   Jacobi). A Dirichlet row of dxo_csr_dirichlet keeps its block invertible. A block with |det| <= 1e-14 of the product
 *                   of its row norms gets a zero inverse and the call returns DXO_E_SINGULAR; it synchronises the stream once for that.
 * dxo_block_jacobi_apply : z = inv r per block of bs (bs = 1: an inverse diagonal, e.g. 1 / dxo_bilinear_diagonal). Capture-safe.
 * dxo_krylov_create : a workspace for vectors of n entries and restart length `restart` (1..64): the basis, four work vectors, the
 *                   Hessenberg matrix and the partials of the reductions, allocated once. The solves allocate nothing.
 * dxo_krylov_gmres : restarted GMRES(restart) with right preconditioning, classical Gram-Schmidt with one reorthogonalisation pass
 *                   (option "krylov_reorth" = 0: one pass). x is the initial guess and is overwritten by the solution. Converged when
 *                   |b - A x| <= max(rtol |b|, atol). The host reads the residual estimate every `check_every` iterations only; the
 *                   update uses the first step whose estimate met the tolerance, so iterations run past it cost time, not accuracy.
 *                   The true residual b - A x is formed with the operator at every restart and at the end. b = 0 gives x = 0 after
 *                   0 iterations. Not converging within max_it is NOT an error: info->converged = 0. Every reduction has a fixed
 *                   shape: a solve is bit-reproducible.
 * dxo_krylov_cg   : preconditioned CG on the same kernels and arguments (A and M symmetric positive definite).
 * dxo_krylov_fgmres : flexible GMRES(restart): the arguments, stopping rule, check_every protocol, breakdown handling and info of
 *                   dxo_krylov_gmres. It keeps z_j = M v_j in a second basis Z [restart][ld], forms w = A z_j and updates
 *                   x += sum_j y_j z_j at the end of a cycle, with no further preconditioner call. M may therefore differ from step
 *                   to step (an inner iteration, a K-cycle); dxo_krylov_gmres and dxo_krylov_cg need a fixed linear M. With a fixed
 *                   M it takes the iterations of dxo_krylov_gmres. The second basis (restart * ld doubles) is allocated at the first
 *                   flexible solve on a workspace and freed with it: a workspace that serves only gmres / cg keeps today's memory.
 * dxo_krylov_create_basis : dxo_krylov_create with the storage of the basis chosen. DXO_KRYLOV_BASIS_FP64 is dxo_krylov_create.
 *                   DXO_KRYLOV_BASIS_FP32 (a compressed basis, as in CB-GMRES) stores the basis as float [restart + 1][ldf], ldf = n
 *                   padded to a multiple of 64 floats, and the work vectors plus two more in double; there is no double basis. Every
 *                   dot product, update, Hessenberg entry, rotation and x stay double: a new basis vector is rounded to float once
 *                   (round to nearest even) and that rounded vector is the one M and A see at the next step, so the Arnoldi relation
 *                   holds for the stored basis. The stopping test is on the double true residual b - A x, formed at every restart, so
 *                   the attainable accuracy is the one of the FP64 basis; the Hessenberg estimate inside a cycle is good to about
 *                   2^-24 of the cycle's starting residual, so a cycle cannot gain much more than seven digits on its own estimate:
 *                   expect at most one extra cycle at tight tolerances. The basis sees normalised vectors only: no range concern.
 *                   dxo_krylov_gmres and dxo_krylov_fgmres take either kind; in dxo_krylov_fgmres the second basis Z stays double
 *                   (the z_j = M v_j are not normalised: their range is the caller's). dxo_krylov_cg keeps no basis and returns
 *                   DXO_E_OPTION on an FP32 workspace; an unknown kind: DXO_E_OPTION. Option "krylov_basis_width": rows of the
 *                   float basis a thread owns in the row kernels (1, 2 or 4).
 * dxo_krylov_basis_info : the kind of a workspace, the bytes of its basis rows alone ((restart + 1) * ld * the element size; the
 *                   second basis of dxo_krylov_fgmres is not counted), the DEVICE pointer of row 0 (float or double by the kind)
 *                   and the row stride in elements. Any out-pointer may be NULL. For tests and reports.
 * Operator: a CSR matrix (csr + values) or a callback that SETS out = A v on the context's stream (e.g. dxo_bilinear_apply with option
 * "consumer_overwrite" = 1). The callback runs on the calling thread while the context's (recursive) lock is held, so it may call
 * other dxo_* entry points on the same context; a nonzero return ends the solve with that code. Preconditioner: NULL or kind
 * DXO_PC_NONE, DXO_PC_JACOBI (inv [n]) or DXO_PC_BLOCK_JACOBI (inv [n/bs][bs][bs], bs equal to the pattern's).
 * DXO_PC_AMG: a dxo_amg (below) after dxo_amg_setup, applied as one cycle; with the K-cycle (dxo_amg_set_cycle) in dxo_krylov_fgmres
 * only: DXO_E_OPTION in the other two.
 * DXO_PC_CALLBACK: inv carries a dxo_krylov_callback* whose function SETS out = M v on the context's stream, under the rules of the
 * operator callback; a nonzero return ends the solve with that code. A NULL struct or function: DXO_E_NULL. bs is ignored.
 * Errors: NULL arguments DXO_E_NULL; operator, matrix, workspace and preconditioner sizes that differ, n not a multiple of bs, max_it < 0 or
 * check_every < 1 DXO_E_SIZE; a preconditioner of another block size DXO_E_DIM; arrays not 8-byte aligned DXO_E_ALIGN; negative
 * tolerances or an unknown preconditioner kind DXO_E_OPTION. */
#define DXO_PC_NONE 0
#define DXO_PC_JACOBI 1
#define DXO_PC_BLOCK_JACOBI 2
#define DXO_PC_AMG 3               /* dxo_krylov_pc::inv carries the dxo_amg* (cast to const double*), bs and n as for block Jacobi */
#define DXO_PC_CALLBACK 4          /* dxo_krylov_pc::inv carries a dxo_krylov_callback* (cast to const double*), n as above        */
#define DXO_KRYLOV_BASIS_FP64 0
#define DXO_KRYLOV_BASIS_FP32 1
typedef struct dxo_krylov dxo_krylov;
typedef int (*dxo_krylov_apply_fn)(void* user, const double* v, double* out);
typedef struct dxo_krylov_op {
    int64_t n;                     /* rows = columns                                      */
    const dxo_csr* csr;            /* a matrix on this pattern ...                        */
    const double* values;          /* ... with these values (nnz)                         */
    dxo_krylov_apply_fn apply;     /* or, with csr NULL, this callback                    */
    void* user;                    /* passed to apply                                     */
} dxo_krylov_op;
typedef struct dxo_krylov_callback {
    dxo_krylov_apply_fn apply;     /* sets out = M v                                      */
    void* user;                    /* passed to apply                                     */
} dxo_krylov_callback;
typedef struct dxo_krylov_pc {
    int kind;                      /* DXO_PC_*                                            */
    int bs;                        /* DXO_PC_BLOCK_JACOBI: block size (1, 2, 3)           */
    int64_t n;                     /* rows the inverse covers: must equal the operator's  */
    const double* inv;             /* inverse diagonal [n] or block inverses [n/bs][bs][bs] */
} dxo_krylov_pc;
typedef struct dxo_krylov_info {
    int32_t iterations;            /* Krylov iterations up to the converged step          */
    int32_t converged;             /* true relative residual met the tolerance            */
    int32_t breakdown;             /* h_{j+1,j} == 0 (GMRES) or (p, A p) == 0 (CG)        */
    int32_t restarts;              /* cycles started                                      */
    double residual;               /* |b - A x| / |b| of the returned x (0 for b = 0)     */
    double ms;                     /* wall time of the solve                              */
} dxo_krylov_info;
int dxo_csr_spmv(dxo_ctx* ctx, const dxo_csr* csr, const double* values, double alpha, const double* x, double beta, double* y);
int dxo_csr_transpose(dxo_ctx* ctx, dxo_csr* csr, const double* values, double* values_t);
int dxo_csr_spmv_t(dxo_ctx* ctx, dxo_csr* csr, const double* values, double alpha, const double* x, double beta, double* y);
int dxo_csr_block_jacobi(dxo_ctx* ctx, const dxo_csr* csr, const double* values, double* inv);
int dxo_block_jacobi_apply(dxo_ctx* ctx, int bs, int64_t n, const double* inv, const double* r, double* z);
int dxo_krylov_create(dxo_ctx* ctx, int64_t n, int restart, dxo_krylov** out);
int dxo_krylov_create_basis(dxo_ctx* ctx, int64_t n, int restart, int basis, dxo_krylov** out);
int dxo_krylov_basis_info(dxo_ctx* ctx, const dxo_krylov* ws, int* basis, int64_t* basis_bytes, const void** rows, int64_t* ld);
int dxo_krylov_destroy(dxo_ctx* ctx, dxo_krylov* ws);
int dxo_krylov_gmres(dxo_ctx* ctx, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b, double* x,
                     double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info);
int dxo_krylov_cg(dxo_ctx* ctx, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b, double* x,
                  double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info);
int dxo_krylov_fgmres(dxo_ctx* ctx, dxo_krylov* ws, const dxo_krylov_op* op, const dxo_krylov_pc* pc, const double* b, double* x,
                      double rtol, double atol, int max_it, int check_every, dxo_krylov_info* info);

/* ---- smoothed-aggregation multigrid preconditioner (csrc/amg.hip), DEVICE memory only ---------------------------
 * A V-cycle for a matrix on a dxo_csr pattern; the block size bs (1, 2, 3) is the same on every level, so every level is a matrix in
 * the layout of dxo_csr_spmv. Nothing but the matrix is needed (no mesh hierarchy).
 * dxo_amg_create  : the symbolic phase, host C++, once per pattern. `constrained` is the DEVICE int32 list given to dxo_csr_dirichlet
 *                   (may be NULL with n_constrained = 0; out-of-range entries are ignored). A node all of whose dofs are constrained
 *                   joins no aggregate. Aggregation in three passes in ascending node order (a node whose whole neighbourhood is free
 *                   founds an aggregate with it; a left-over node joins the lowest pass-1 aggregate among its neighbours; the rest
 *                   found aggregates with their free neighbours): a function of the pattern and the list alone. Block patterns of
 *                   P, A P and P^T A P and the transposed incidence of P are built and uploaded; the coarse patterns are dxo_csr
 *                   objects without a mesh (dxo_bilinear_assemble and dxo_csr_dirichlet answer DXO_E_DIM on them). Coarsening stops at
 *                   n_rows <= coarse_rows, at max_levels, or when a coarse level would keep more than 0.8 of its parent's rows. A
 *                   coarsest level of more than 4096 rows: DXO_E_SIZE. max_levels, coarse_rows or sweeps < 1: DXO_E_SIZE; bs outside
 *                   1..3: DXO_E_DIM. All device memory of setup and apply is allocated here.
 * dxo_amg_setup   : the numeric phase for the matrix `values` on the pattern of the creation, on the context's stream: per level the
 *                   block-Jacobi inverses, rho = |Dinv A|_inf (or the estimate chosen by dxo_amg_set_smoother, below) and
 *                   omega = (4/3) / rho (kept on the device), P = T - omega Dinv A T,
 *                   A_c = P^T (A P); the coarsest matrix is inverted densely (Gauss-Jordan, partial pivoting). Sums run in ascending
 *                   source order, no atomics: two setups from the same values give bit-identical hierarchies. One synchronisation at
 *                   the end reads one flag: a singular diagonal block or a zero pivot gives DXO_E_SINGULAR. `values` is read again by
 *                   dxo_amg_apply and must stay alive and unchanged until the next setup.
 * dxo_amg_apply   : z = V(r): `sweeps` damped block-Jacobi sweeps before and after the coarse correction on every level (the first
 *                   from x = 0), restriction by P^T, the dense inverse on the coarsest level. r may equal z. A fixed linear operator,
 *                   symmetric for a symmetric matrix. Capture-safe, allocation-free, bit-reproducible. Before a successful setup:
 *                   DXO_E_OPTION.
 * dxo_amg_info    : counts and the DEVICE arrays of one level (any pointer may be NULL; `level` outside [0, n_levels): DXO_E_SIZE).
 * In dxo_krylov_gmres / dxo_krylov_cg: kind DXO_PC_AMG, inv = (const double*)amg, bs and n those of the matrix; an object made for a
 * pattern of another size is DXO_E_SIZE, of another block size DXO_E_DIM, one without a setup DXO_E_OPTION.
 *
 * With a near-null space (elasticity: the rigid-body modes) the coarse spaces carry rotations as well as translations:
 * dxo_rigid_body_modes : B [n_nodes * gdim][k] from node coordinates x [n_nodes][gdim] (both DEVICE), k = 3 for gdim 2, 6 for gdim 3:
 *                   the gdim translations, then (-y, x) in 2-D and (-y, x, 0), (0, -z, y), (z, 0, -x) in 3-D. The coordinates are
 *                   used as given. gdim outside 2..3: DXO_E_DIM. Capture-safe.
 * dxo_amg_create_nns : dxo_amg_create with the near-null space B [n_rows][n_modes] (DEVICE, copied); (bs, n_modes) must be (2, 3) or
 *                   (3, 6): DXO_E_DIM otherwise; B not 8-byte aligned: DXO_E_ALIGN. Non-finite entries are the caller's problem. The
 *                   rows of B of constrained dofs are set to zero. The aggregates and all block patterns are those of
 *                   dxo_amg_create. Per level and aggregate the rows of B of its nodes (ascending) are orthonormalised on the
 *                   device (Gram-Schmidt in column order with a second pass); the Q factors are the blocks of the tentative
 *                   prolongator T (bs_l x n_modes per node), the R factors the B of the next level. A column that keeps no more
 *                   than 10^-n of its norm (option "amg_rank_tol" = n, default 10) is dead: its column of Q and its row of the next
 *                   B are zero, its coarse diagonal entry becomes 1. Every coarse level has block size n_modes; the coarsening
 *                   stops when a level would keep more than 0.8 of its parent's rows (n_aggregates * n_modes rows). T and B are
 *                   made once, here; dxo_amg_setup, dxo_amg_apply and dxo_amg_destroy are used as before and have the same
 *                   properties. In dxo_amg_level_info n_rows, nnz_blocks, dinv and p_values describe a level with its own block
 *                   size: dinv [n_nodes][bs_l][bs_l], p_values [p_blocks][bs_l][bs_coarse].
 * dxo_amg_nns_info : the block size of `level` and of the next one, the dead columns of its T, and the DEVICE arrays T
 *                   [n_nodes][bs][bs_coarse] (NULL on the coarsest level) and B [n_rows][n_modes]; any pointer may be NULL. On an
 *                   object of dxo_amg_create: bs_coarse = bs, 0 dead columns, NULL arrays.
 *
 * The relaxation (every object starts with DXO_AMG_SMOOTH_JACOBI and DXO_AMG_RHO_INF_NORM, which is all of the above):
 * dxo_amg_set_smoother : the smoother and the source of rho for the NEXT dxo_amg_setup; until then dxo_amg_apply and the Krylov calls
 *                   answer DXO_E_OPTION. rho_kind DXO_AMG_RHO_POWER: rho = safety * |w_m|, m = rho_iters steps
 *                   w_k = Dinv A (w_{k-1} / |w_{k-1}|) from w_0[i] = 0.5 + ((uint32)(i * 2654435761) >> 8) * 2^-24 on every level, on
 *                   the device, with fixed reduction orders (bit-reproducible, no additional synchronisation). It is an estimate of
 *                   the spectral radius from below times `safety`, not a bound. omega = (4/3) / rho of the prolongator smoothing and
 *                   of the Jacobi sweeps follows the selected rho. kind DXO_AMG_SMOOTH_CHEBYSHEV: the `sweeps` Jacobi sweeps before
 *                   and after the coarse correction become the Chebyshev polynomial of `degree` (1..8) in Dinv A on
 *                   [lower * rho, rho]: with theta = (1 + lower) rho / 2, delta = (1 - lower) rho / 2, sigma = theta / delta:
 *                   rho_0 = 1 / sigma, d = Dinv res / theta, x += d; then rho_1 = 1 / (2 sigma - rho_0),
 *                   d = rho_1 rho_0 d + (2 rho_1 / delta) Dinv (r - A x), x += d, rho_0 = rho_1. The post-smoothing is the same
 *                   polynomial from the corrected x, so the cycle stays symmetric for a symmetric matrix. Chebyshev with
 *                   DXO_AMG_RHO_INF_NORM is allowed (a wide interval). For DXO_AMG_SMOOTH_JACOBI `degree` is ignored. Unknown kinds,
 *                   Chebyshev degree outside 1..8, rho_iters < 1, lower outside (0, 1), safety < 1: DXO_E_OPTION, nothing changes.
 *                   Allocates nothing: the one extra vector per level was allocated at creation.
 * dxo_amg_smoother_info : the settings (degree: `sweeps` for Jacobi) and the DEVICE address of the rho of `level` that omega was made
 *                   from at the last setup, under either estimate (NULL on the coarsest level); any pointer may be NULL.
 *
 * Strength of connection (anisotropic operators, stretched cells): coarsen only along strong couplings.
 * dxo_amg_create_soc : dxo_amg_create (B NULL, n_modes 0) or dxo_amg_create_nns with the threshold theta and the matrix `values`
 *                   (DEVICE, on the pattern of csr). theta == 0: the object of those two calls bit for bit, `values` is not read.
 *                   theta > 0: block (i, j), i != j, of a level is strong when |A_ij|_F^2 >= theta^2 |A_ii|_F |A_jj|_F or the same
 *                   holds for (j, i) (an absent transposed block: the one-sided test); the squares are summed entry by entry in
 *                   row-major order and compared in double, on entries multiplied by a power of two (|A_ii|_F: by the exponent of
 *                   the block's largest entry; a comparison: by that of the larger of the two norms), so the mask does not depend
 *                   on the scale of the matrix wherever its entries are finite. Diagonal blocks are strong. The aggregates are those of the three
 *                   passes on the strong graph (a node without a strong neighbour founds an aggregate of its own in pass 1), P has
 *                   the pattern (strong graph) x (aggregates), A P and P^T A P are built from the full graph. Because the mask of a
 *                   coarse level needs the coarse matrix, creation runs the numeric phase of every level as it goes (one
 *                   synchronisation per level, here only), with the default relaxation (Jacobi, infinity norm). The masks, the
 *                   aggregates and all patterns are frozen at creation: dxo_amg_setup (still required before the first apply, still
 *                   device-only, allocation-free and single-wait) reuses them for new values, and a later dxo_amg_set_smoother
 *                   changes omega but not the masks. In every setup the prolongator is P = T - omega_F Dinv_F A^F T with A^F the
 *                   matrix without its weak blocks, each added onto the diagonal block of its row in ascending column order (never
 *                   stored), Dinv_F the inverses of those lumped blocks, omega_F = (4/3) / rho_F and rho_F the selected estimate
 *                   (infinity norm or power iteration) of Dinv_F A^F. A lumped block that fails the singularity test of
 *                   dxo_csr_block_jacobi is replaced by A_ii in Dinv_F for that node (counted); a node without a strong
 *                   off-diagonal block is not smoothed: its row of P is its row of T. The sweeps and the Chebyshev smoother keep A,
 *                   Dinv and rho. The stopping rules are those of dxo_amg_create; a theta that leaves nothing strong gives one
 *                   level (DXO_E_SIZE above 4096 rows). theta < 0, >= 1 or not finite: DXO_E_OPTION; values NULL: DXO_E_NULL;
 *                   values or B misaligned: DXO_E_ALIGN; a singular diagonal block met on the way: DXO_E_SINGULAR.
 * dxo_amg_soc_info : theta, the DEVICE mask of `level` (one uint8 per block, in the order of the level's block pattern), its number
 *                   of strong blocks, the nodes whose lumped block failed the test at the last setup (waits for the stream), and
 *                   the DEVICE arrays dinv_f [n_nodes][bs][bs] and omega_F (one double). Any pointer may be NULL. On an object made
 *                   without strength, and on the coarsest level: NULL arrays, every block strong, 0 nodes; theta is the object's.
 *
 * The cycle (every object starts with DXO_AMG_CYCLE_V):
 * dxo_amg_set_cycle : DXO_AMG_CYCLE_V or DXO_AMG_CYCLE_K, on any hierarchy and relaxation; it takes effect at once, without a setup.
 *                   K-cycle: level 0 runs one cycle body B_0 (pre-smoothing, restriction, coarse solve, prolongation,
 *                   post-smoothing), the coarsest level keeps its dense solve, and on every level l between them A_l x = r is
 *                   solved by exactly two GCR steps preconditioned by B_l: c1 = B_l(r), v1 = A_l c1, rho1 = (v1, v1), a1 = (v1, r),
 *                   r1 = r - (a1 / rho1) v1, c2 = B_l(r1), v2 = A_l c2, g = (v2, v1), beta = (v2, v2), a2 = (v2, r1),
 *                   rho2 = beta - g (g / rho1), x2 = a2 / rho2, x = (a1 / rho1 - (g / rho1) x2) c1 + x2 c2. rho1 == 0: x = 0; rho2
 *                   not finite or <= 1e-14 beta: x = (a1 / rho1) c1. The coefficients are ratios of dot products; no product of two
 *                   dot products is formed. An apply is therefore homogeneous of degree one in r, bit for bit, as long as the dot
 *                   products themselves, second powers of |r|, are finite and normal: |r| roughly within 2^-500 .. 2^500 (the
 *                   V-cycle is linear over the whole range of double). Both steps always run (no early exit after the first), the
 *                   coefficients stay on the device: dxo_amg_apply remains capture-safe, allocation-free and bit-reproducible, but
 *                   is no longer a linear operator, so dxo_krylov_gmres / dxo_krylov_cg refuse the object (DXO_E_OPTION) and
 *                   dxo_krylov_fgmres takes it. With at most two levels K is V bit for bit. The first DXO_AMG_CYCLE_K allocates
 *                   five vectors per intermediate level. An unknown kind: DXO_E_OPTION, nothing changes.
 * dxo_amg_cycle_info : the kind, and the level visits of one apply: the levels for V; for K 2^l per level l but the coarsest, which
 *                   is visited as often as the level above it. Any pointer may be NULL.
 *
 * The precision of the cycle (every object starts with DXO_AMG_PRECISION_FP64, which is all of the above bit for bit):
 * dxo_amg_set_precision : the scalar of the cycle for the NEXT dxo_amg_setup; until then dxo_amg_apply and the Krylov calls answer
 *                   DXO_E_OPTION (setting the kind the object already has does nothing). DXO_AMG_PRECISION_FP32: dxo_amg_setup stays
 *                   double to its end (inverses, omega, rho, the Chebyshev pairs, P, A P, P^T A P, the dense inverse, the strength
 *                   and near-null-space paths) and then casts, per level but the coarsest, the level's values (level 0: the
 *                   caller's), dinv and the values of P to float, before its one synchronisation. A finite entry that leaves the
 *                   range of float: DXO_E_OPTION with the level in the message; underflow to zero is not an error. dxo_amg_apply then
 *                   runs the launch sequence of the V-cycle with these copies, float vectors and float fused multiply-adds in the
 *                   same order; omega and the Chebyshev pairs are read as double and narrowed; the coarsest level keeps its double
 *                   dense inverse (right-hand side widened, result narrowed). r and z stay double: r is narrowed by one pass on
 *                   entry (r may still be z), so an |r| beyond the range of float (about 2^-126 .. 2^127; smaller entries lose
 *                   bits, then become 0, larger ones infinite) is not representable and must be scaled by the caller; the last post-smoothing sweep of level 0 writes z. No host read, no allocation, no
 *                   atomics: capture-safe and bit-reproducible as before, and a fixed linear operator up to single-precision
 *                   rounding, so dxo_krylov_gmres, dxo_krylov_cg and dxo_krylov_fgmres all take it (their own arithmetic stays
 *                   double; dxo_krylov_fgmres is the natural partner, dxo_krylov_gmres may spend one more restart below 1e-7).
 *                   A hierarchy of one level is its dense product in double under either kind. The first
 *                   DXO_AMG_PRECISION_FP32 allocates the copies and five float vectors per level (two on the coarsest); they stay
 *                   with the object. The K-cycle is double only: DXO_AMG_PRECISION_FP32 on an object with DXO_AMG_CYCLE_K, and
 *                   dxo_amg_set_cycle(DXO_AMG_CYCLE_K) on an object with DXO_AMG_PRECISION_FP32, answer DXO_E_OPTION and change
 *                   nothing. An unknown kind: DXO_E_OPTION.
 * dxo_amg_precision_info : the kind, and the bytes of the single-precision copies and vectors (0 if none were ever allocated). Any
 *                   pointer may be NULL.
 *
 * A given first transfer (quadratic elements: coarsen in the polynomial degree before aggregating):
 * dxo_amg_create_transfer : dxo_amg_create_soc with the prolongator of level 0 given as a nodal interpolation P = W (x) I_bs
 *                   (`first`, HOST arrays, copied; NULL: dxo_amg_create_soc exactly). W [n_nodes][n_coarse] in CSR form: row i holds
 *                   the coarse nodes (ascending) and weights of fine node i; coarse node v IS the fine node coarse_to_fine[v], whose
 *                   row is the single entry (v, 1). Level 0 keeps all a level smooths with (dinv, rho, omega, the Chebyshev pairs);
 *                   its P is stored as the diagonals of its blocks, p_diag [p_blocks][bs] = w_iv keep(i, c) keep(coarse_to_fine[v], c)
 *                   with keep 0 for a constrained dof, frozen here; a setup forms A_1 = P^T A P on the symbolic pattern of the
 *                   product (an exactly zero diagonal entry becomes 1) and builds no P, mask or filtered matrix on level 0. Level 1
 *                   is treated as a finest level: its constrained set is that of the nodes coarse_to_fine (a node with all dofs
 *                   constrained joins no aggregate, the mask of T is this set, not a values-dependent one), its near-null space is
 *                   the rows of the zeroed B at coarse_to_fine (exact for rigid-body modes under a degree-1 interpolation), and
 *                   theta takes effect from level 1. Levels 1... are bit for bit the hierarchy the library builds from A_1 and that
 *                   set. dxo_amg_set_smoother, dxo_amg_set_cycle and dxo_amg_set_precision apply as before (single precision: a float
 *                   copy of p_diag). In dxo_amg_level_info of level 0 aggregate and p_values are NULL and n_aggregates is n_coarse;
 *                   dxo_amg_nns_info reports bs_coarse = bs there. If level 0 is already the coarsest (n_rows <= coarse_rows,
 *                   max_levels 1) the transfer is checked and not used. Errors beyond those of dxo_amg_create_soc: a NULL array
 *                   DXO_E_NULL; n_coarse < 1 or n_coarse * bs above 0.8 n_rows (the stagnation rule), ptr[0] != 0, a node without an
 *                   entry, a column or a coarse_to_fine outside its range: DXO_E_SIZE; columns of a row not ascending, a weight not
 *                   finite, coarse_to_fine naming a node twice, a row of coarse_to_fine[v] other than {(v, 1.0)}: DXO_E_OPTION.
 * dxo_amg_transfer_info : whether level 0 carries a given transfer, its coarse nodes and blocks, and the DEVICE arrays p_diag
 *                   [p_blocks][bs] and coarse_to_fine [n_coarse] (0 / NULL without one). Any pointer may be NULL. */
enum { DXO_AMG_PRECISION_FP64 = 0, DXO_AMG_PRECISION_FP32 = 1 };
#define DXO_AMG_SMOOTH_JACOBI 0
#define DXO_AMG_SMOOTH_CHEBYSHEV 1
#define DXO_AMG_RHO_INF_NORM 0
#define DXO_AMG_RHO_POWER 1
#define DXO_AMG_CYCLE_V 0
#define DXO_AMG_CYCLE_K 1
typedef struct dxo_amg dxo_amg;
typedef struct dxo_amg_level_info {
    int64_t n_rows, n_nodes;       /* of A_l                                              */
    int64_t nnz_blocks;            /* bs x bs blocks of A_l                               */
    const dxo_csr* csr;            /* pattern of A_l (level 0: the caller's)              */
    const double* values;          /* A_l (level 0: the pointer of the last setup)        */
    const double* dinv;            /* [n_nodes][bs][bs]; NULL on the coarsest level       */
    const double* omega;           /* one double on the device; NULL on the coarsest      */
    int64_t n_aggregates;          /* nodes of level l + 1; 0 on the coarsest level       */
    const int32_t* aggregate;      /* [n_nodes] aggregate of a node, -1: none             */
    int64_t p_blocks;              /* blocks of P_l, block CSR over nodes x aggregates    */
    const int64_t* p_ptr;          /* [n_nodes + 1]                                       */
    const int32_t* p_col;          /* [p_blocks] aggregate                                */
    const double* p_values;        /* [p_blocks][bs][bs]                                  */
    int64_t ap_blocks;             /* blocks of A_l P_l                                   */
    const int64_t* ap_ptr;         /* [n_nodes + 1]                                       */
    const int32_t* ap_col;         /* [ap_blocks]                                         */
} dxo_amg_level_info;
int dxo_amg_create(dxo_ctx* ctx, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained, int max_levels, int coarse_rows,
                   int sweeps, dxo_amg** out);
int dxo_amg_destroy(dxo_ctx* ctx, dxo_amg* amg);
int dxo_amg_setup(dxo_ctx* ctx, dxo_amg* amg, const double* values);
int dxo_amg_apply(dxo_ctx* ctx, dxo_amg* amg, const double* r, double* z);
int dxo_amg_info(dxo_ctx* ctx, const dxo_amg* amg, int* n_levels, double* build_ms, double* operator_complexity, int level,
                 dxo_amg_level_info* out);
int dxo_rigid_body_modes(dxo_ctx* ctx, const double* x, int64_t n_nodes, int gdim, double* B);
int dxo_amg_create_nns(dxo_ctx* ctx, const dxo_csr* csr, const int32_t* constrained, int64_t n_constrained, const double* B, int n_modes,
                       int max_levels, int coarse_rows, int sweeps, dxo_amg** out);
int dxo_amg_nns_info(dxo_ctx* ctx, const dxo_amg* amg, int level, int* bs, int* bs_coarse, int64_t* dead_columns, const double** t_val,
                     const double** b_val);
int dxo_amg_set_smoother(dxo_ctx* ctx, dxo_amg* amg, int kind, int degree, int rho_kind, int rho_iters, double lower, double safety);
int dxo_amg_smoother_info(dxo_ctx* ctx, const dxo_amg* amg, int level, int* kind, int* degree, int* rho_kind, int* rho_iters,
                          const double** rho);
int dxo_amg_create_soc(dxo_ctx* ctx, const dxo_csr* csr, const double* values, const int32_t* constrained, int64_t n_constrained,
                       const double* B, int n_modes, double theta, int max_levels, int coarse_rows, int sweeps, dxo_amg** out);
int dxo_amg_soc_info(dxo_ctx* ctx, const dxo_amg* amg, int level, double* theta, const uint8_t** strong, int64_t* n_strong_blocks,
                     int64_t* n_unlumped_nodes, const double** dinv_f, const double** omega_f);
int dxo_amg_set_cycle(dxo_ctx* ctx, dxo_amg* amg, int kind);
int dxo_amg_cycle_info(dxo_ctx* ctx, const dxo_amg* amg, int* kind, int64_t* visits);
int dxo_amg_set_precision(dxo_ctx* ctx, dxo_amg* amg, int kind);
int dxo_amg_precision_info(dxo_ctx* ctx, const dxo_amg* amg, int* kind, int64_t* fp32_bytes);
typedef struct dxo_amg_transfer {  /* host arrays, copied at creation                       */
    int64_t n_coarse;              /* coarse nodes                                           */
    const int64_t* ptr;            /* [n_nodes + 1] rows of W                                */
    const int32_t* col;            /* coarse nodes of a row, ascending                       */
    const double* w;               /* weights                                                */
    const int32_t* coarse_to_fine; /* [n_coarse] the fine node a coarse node is              */
} dxo_amg_transfer;
int dxo_amg_create_transfer(dxo_ctx* ctx, const dxo_csr* csr, const double* values, const int32_t* constrained, int64_t n_constrained,
                            const double* B, int n_modes, double theta, const dxo_amg_transfer* first, int max_levels, int coarse_rows,
                            int sweeps, dxo_amg** out);
int dxo_amg_transfer_info(dxo_ctx* ctx, const dxo_amg* amg, int* present, int64_t* n_coarse, int64_t* p_blocks, const double** p_diag,
                          const int32_t** coarse_to_fine);

/* ---- p-multigrid on an operator (csrc/pmg.hip), DEVICE memory only ------------------------------------------------
 * A two-level cycle for quadratic elements whose finest level is an OPERATOR (a dxo_krylov_op: a matrix, or a callback such as
 * dxo_isihara3_tangent_apply), never a matrix: Chebyshev smoothing in Dinv A with the inverse DIAGONAL alone, restriction of the
 * residual to the degree-1 space on the same cells by a nodal interpolation (dxo_amg_transfer, DeviceMesh.vertex_transfer), any
 * preconditioner of a matrix of that space (usually a dxo_amg of the rediscretised degree-1 matrix, which for nested Lagrange spaces,
 * the same rule and the same coefficients is P^T A P to rounding), prolongation, and the same polynomial again. bs is 1, 2 or 3.
 * dxo_pmg_create  : the symbolic part, host C++, once per mesh. `transfer` (HOST arrays, copied) is checked by the rules of
 *                   dxo_amg_create_transfer with its error codes, but for the stagnation rule of the multigrid's coarsening, which
 *                   says nothing about a transfer (n_coarse above n_nodes: DXO_E_SIZE). `constrained` is the DEVICE int32 list given to
 *                   dxo_csr_dirichlet (NULL with n_constrained = 0; out-of-range entries are ignored). The prolongator P = W (x) I_bs
 *                   is stored as dxo_amg_create_transfer stores it, p_diag [block][bs] = w_iv keep(i, c) keep(coarse_to_fine[v], c),
 *                   with its transposed incidence (coarse node -> its blocks, fine nodes ascending), so that the restriction is a
 *                   gather without atomics. The constrained dofs of the coarse space are listed too (ascending): dof (v, c) iff fine
 *                   dof (coarse_to_fine[v], c) is constrained; hand the list to the assembly of the coarse matrix as its Dirichlet
 *                   set. All device memory of setup and apply is allocated here: four fine vectors (x, d, t and the vector of the
 *                   power iteration), the coarse right-hand side and correction. bs outside 1..3: DXO_E_DIM; n_nodes or
 *                   n_constrained < 0, 2^31 dofs or more: DXO_E_SIZE.
 * dxo_pmg_set_smoother : degree (1..8) of the Chebyshev polynomial, the steps of the power iteration, and `lower`, `safety` as in
 *                   dxo_amg_set_smoother (defaults 2, 10, 0.1, 1.1; the same ranges, DXO_E_OPTION and nothing changes). It takes
 *                   effect at the NEXT dxo_pmg_setup; until then dxo_pmg_apply and the Krylov calls answer DXO_E_OPTION.
 * dxo_pmg_setup   : `fine` is the operator (csr + values, bs that of the object, or a callback that SETS out = A v), n = n_nodes * bs;
 *                   `dinv` [n] its inverse diagonal with 1 on constrained dofs, where the operator must be the identity; `coarse` a
 *                   preconditioner of n_coarse * bs rows: DXO_PC_AMG (V-cycle; a K-cycle: DXO_E_OPTION), DXO_PC_BLOCK_JACOBI,
 *                   DXO_PC_JACOBI or DXO_PC_CALLBACK (the struct is copied); DXO_PC_NONE and unknown kinds: DXO_E_OPTION. rho is the
 *                   power estimate of Dinv A documented at dxo_amg_set_smoother: w_0[i] = 0.5 + ((uint32)(i * 2654435761) >> 8) * 2^-24,
 *                   rho_iters steps w_k = Dinv A (w_{k-1} / |w_{k-1}|), rho = safety |w_m|. |w|^2 is summed on a grid that depends on n
 *                   alone (min(1024, ceil(n / 256)) workgroups of 256: a thread adds its entries in ascending order, then the
 *                   xor-butterfly of the wave, then the four waves in ascending order; one workgroup adds the partials likewise), so
 *                   rho is bit-reproducible. rho stays on the device and the `degree` pairs (c1, c2) are formed from it there by the
 *                   recurrence at dxo_amg_set_smoother (rho not > 0: all-zero pairs): no host read, no synchronisation. Costs
 *                   rho_iters operator calls. fine, dinv and coarse (and what they point to) are used again by every apply: they must
 *                   stay alive and unchanged until the next setup. Sizes that differ: DXO_E_SIZE; a matrix or a coarse object of
 *                   another block size: DXO_E_DIM; NULLs DXO_E_NULL; misaligned arrays DXO_E_ALIGN; a failing callback: its code.
 * dxo_pmg_apply   : z = M r. (1) x = the polynomial from x = 0; its first step is d = c2 dinv r, x = d, without an operator call or a
 *                   memset: degree - 1 calls. (2) t = A x, r_c = P^T (r - t), the subtraction inside the restriction. (3) e_c =
 *                   coarse(r_c). (4) x += P e_c. (5) the same polynomial from the corrected x, d = c1 d + c2 dinv (r - A x),
 *                   x += d, the last step writing z: degree calls. 2 degree operator calls in all. r may equal z. M is a fixed linear
 *                   operator, symmetric for a symmetric A and a symmetric coarse preconditioner, homogeneous bit for bit under
 *                   powers of two. Allocation-free, atomic-free, bit-reproducible, and capture-safe wherever the operator and the
 *                   coarse preconditioner are. Before a successful setup: DXO_E_OPTION. Option "pmg_grid_blocks": the most
 *                   workgroups of 256 an elementwise or transfer kernel is launched with (0, the default: 16 per compute unit;
 *                   1..65535); beyond it a thread strides. Every entry is formed by one thread alone, so no result depends on it.
 * dxo_pmg_restrict / dxo_pmg_prolong : the transfers alone. Restriction SETS r_c[v][c] = sum_i p_diag r[i][c] over the fine nodes of
 *                   column v in ascending i; prolongation SETS x[i][c] = sum_v p_diag e[v][c] over the coarse nodes of row i in
 *                   ascending v (inside the cycle it accumulates onto x in the same order).
 * dxo_pmg_info    : the coarse rows, the blocks of P, and the DEVICE arrays p_diag [p_blocks][bs], the coarse constrained list (int32)
 *                   with its length, rho (one double), the pairs [degree][2]; the degree set, and the operator calls of one apply
 *                   (2 degree). Any out-pointer may be NULL.
 * In dxo_krylov_gmres / dxo_krylov_cg / dxo_krylov_fgmres: kind DXO_PC_PMG, inv = (const double*)pmg, n that of the operator (bs is
 * ignored); another size DXO_E_SIZE, a matrix operator of another block size DXO_E_DIM, no valid setup DXO_E_OPTION. inv is checked
 * against the live objects of dxo_pmg_create before it is read: any other pointer under this kind is DXO_E_OPTION, as an unknown kind
 * is (dxo_pmg_destroy answers the same for such a pointer, a second destroy included). */
typedef struct dxo_pmg dxo_pmg;
int dxo_pmg_create(dxo_ctx* ctx, int64_t n_nodes, int bs, const dxo_amg_transfer* transfer, const int32_t* constrained, int64_t n_constrained,
                   dxo_pmg** out);
int dxo_pmg_destroy(dxo_ctx* ctx, dxo_pmg* pmg);
int dxo_pmg_set_smoother(dxo_ctx* ctx, dxo_pmg* pmg, int degree, int rho_iters, double lower, double safety);
int dxo_pmg_setup(dxo_ctx* ctx, dxo_pmg* pmg, const dxo_krylov_op* fine, const double* dinv, const dxo_krylov_pc* coarse);
int dxo_pmg_apply(dxo_ctx* ctx, dxo_pmg* pmg, const double* r, double* z);
int dxo_pmg_restrict(dxo_ctx* ctx, dxo_pmg* pmg, const double* r_fine, double* r_coarse);
int dxo_pmg_prolong(dxo_ctx* ctx, dxo_pmg* pmg, const double* e_coarse, double* x_fine);
int dxo_pmg_info(dxo_ctx* ctx, const dxo_pmg* pmg, int64_t* n_coarse_rows, int64_t* p_blocks, const double** p_diag,
                 const int32_t** coarse_constrained, int64_t* n_coarse_constrained, const double** rho, const double** pairs, int* degree,
                 int64_t* matvecs_per_apply);
#define DXO_PC_PMG 5               /* dxo_krylov_pc::inv carries the dxo_pmg* (cast to const double*), n as for the other kinds    */

/* ---- boundary-facet integrals (ds) on the device: loads of a residual F = ... - inner(t, v) ds --------------------------
 * The demo's residual inner(sigma, eps(v)) dx - inner(loading * -n, v) ds(inner) (demo_plasticity_von_mises.py:249-253) is
 * dxo_operand_adjoint(EPS_MANDEL) followed by dxo_facet_pressure(scale = loading) on the facets of the tag.
 * dxo_mesh_set_facet_geometry : reference facet data, one entry per LOCAL facet, matching the facet tables (dxo_mesh_set_facet_tables
 *     first: DXO_E_OPTION otherwise; n_local_facets and nq must equal the tables': DXO_E_DIM otherwise). Host pointers, copied:
 *       weights       [nq]                reference facet quadrature weights (basix.make_quadrature(facet_cell, deg)[1])
 *       ref_normals   [nf][gdim]          outward unit normals of the reference cell (basix.cell.facet_outward_normals)
 *       ref_jacobians [nf][gdim][gdim-1]  reference facet -> reference cell Jacobians (basix.cell.facet_jacobians)
 * dxo_facet_set_create : a fixed list of (cell, local facet) entities (host int32 [n][2], e.g. the facets of one tag), built ONCE:
 *     validated (outside [0, num_cells) x [0, n_local_facets): DXO_E_SIZE; facet tables not set: DXO_E_OPTION), copied to the device,
 *     with the element-vector scratch and the transposed incidence node -> (entity, local dof) in ascending entity order. The
 *     calls below allocate nothing and synchronise nothing: they are capture-safe once the set exists.
 * Geometry at a facet point: J is rebuilt from the facet dpsi table exactly as dxo_eval_operand_facets does; J_f = J J_ref_f,
 *     dS = w_q sqrt(det(J_f^T J_f)) (the point measure of ds), n = J^-T n_ref / |J^-T n_ref| — outward whatever the sign of det J.
 * dxo_eval_facet_geometry : UFL's FacetNormal and dS at the facet points, DEVICE pointers; either may be NULL.
 *     normals [n][nq][gdim], dS [n][nq].
 * dxo_facet_adjoint : out[dof] += sum_e sum_q dS_eq B_eq^T S_eq, the facet adjoint of dxo_eval_operand_facets for the linear kinds and
 *     block sizes dxo_operand_adjoint takes (VALUE, GRAD, VALUE_GRAD with bs = 1 or gdim; EPS_MANDEL, DIV, DEFGRAD (as its
 *     linearisation, grad) with bs = gdim); S [n][nq][value_size]. Nonlinear kinds (C, I1, det F): DXO_E_OPTION. VALUE with bs = gdim
 *     and S = t is the load vector of a traction t.
 * dxo_facet_pressure : out[node*gdim + i] += scale * sum_e sum_q dS_eq p_eq phi_a(x_eq) n_i(x_eq), p [n][nq] or NULL for p = 1, n the
 *     outward unit normal formed in the kernel.
 * The facet calls always ACCUMULATE into out: options "consumer_overwrite" and "adjoint_atomics" do not apply to them. Element vectors
 * go to the set's scratch, then one lane per touched node adds that node's entries in ascending entity order: no atomics,
 * bit-reproducible. Facet geometry not set: DXO_E_OPTION; a set created on another mesh, or tables / geometry changed to another
 * (nf, nq) since: DXO_E_DIM; NULL arrays DXO_E_NULL, arrays not 8-byte aligned DXO_E_ALIGN. */
int dxo_mesh_set_facet_geometry(dxo_ctx* ctx, dxo_mesh* mesh, int n_local_facets, int nq, const double* weights,
                                const double* ref_normals, const double* ref_jacobians);
typedef struct dxo_facet_set dxo_facet_set;
int dxo_facet_set_create(dxo_ctx* ctx, dxo_mesh* mesh, const int32_t* entities, int64_t n, dxo_facet_set** out);
int dxo_facet_set_destroy(dxo_ctx* ctx, dxo_facet_set* set);
int dxo_eval_facet_geometry(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_facet_set* set, double* normals, double* dS);
int dxo_facet_adjoint(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_facet_set* set, int kind, int bs, const double* S, double* out);
int dxo_facet_pressure(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_facet_set* set, const double* p, double scale, double* out);

/* ---- bilinear forms on boundary facets: the Jacobian of a boundary term g(operand(u)) . v ds --------------------------
 * The derivative of a state-dependent boundary load with respect to u, int (dg/d operand . operand(u_hat)) . v ds (a convective or
 * radiative flux, an elastic foundation, a traction that depends on u or grad u):
 *   K[(a,i),(b,j)] = sum_e sum_q dS_eq phi_a(x_eq) sum_r C_eq[i][r] (B_trial,eq)_r,(b,j)
 * over the set's entities, dS and the facet tables exactly those of dxo_facet_adjoint. All pointers are DEVICE pointers, 8-byte aligned
 * (DXO_E_ALIGN otherwise). C [n][nq_facet][bs][D_trial] row-major, D_trial = dxo_operand_value_size(gdim, bs, trial_kind).
 * test_kind must be DXO_OPERAND_VALUE (any other: DXO_E_OPTION). trial_kind: the linear kinds of dxo_facet_adjoint with its block sizes
 * (VALUE, GRAD, VALUE_GRAD with bs = 1 or gdim; EPS_MANDEL, DIV, DEFGRAD — taken as its linearisation, grad — with bs = gdim);
 * nonlinear kinds DXO_E_OPTION, a block size that does not fit DXO_E_DIM.
 *   dxo_facet_bilinear_apply    : out += K v
 *   dxo_facet_bilinear_diagonal : out += diag K
 *   dxo_facet_bilinear_assemble : values += K on a pattern of dxo_csr_create(mesh, bs) (of another mesh or block size: DXO_E_DIM)
 * Like the other facet calls they ALWAYS accumulate ("consumer_overwrite" and "adjoint_atomics" do not apply: the facet term goes on
 * top of a cell term), use no atomics and are bit-reproducible: apply and diagonal write element vectors to the set's scratch and
 * finish with the node sums of dxo_facet_adjoint; assemble writes the element matrices of a chunk of entities (option
 * "assemble_chunk_cells" entities, 0 = as many as fit 1 GiB) to a grow-only scratch of the set that the first call allocates, then one
 * lane per (touched node, component) adds that row's entries in ascending entity order: every value is the same chain of additions
 * whatever the chunk size. After that first call they allocate and synchronise nothing (capture-safe). An empty set: DXO_OK, nothing
 * touched. dxo_facet_bilinear_assemble parks nq_facet blocks of bs * bs * (1 | gdim | 1 + gdim) doubles (rounded up to odd) per entity
 * in LDS: a facet rule so large that ONE entity exceeds 64 KiB (nq_facet >= 222 with value_grad, bs = gdim = 3) is refused with
 * DXO_E_SIZE. The other checks and codes are those of dxo_facet_adjoint. */
int dxo_facet_bilinear_apply(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_facet_set* set, int test_kind, int trial_kind, int bs, const double* C,
                             const double* v, double* out);
int dxo_facet_bilinear_diagonal(dxo_ctx* ctx, dxo_mesh* mesh, const dxo_facet_set* set, int test_kind, int trial_kind, int bs,
                                const double* C, double* out);
int dxo_facet_bilinear_assemble(dxo_ctx* ctx, dxo_mesh* mesh, dxo_facet_set* set, dxo_csr* csr, int test_kind, int trial_kind, int bs,
                                const double* C, double* values);

/* ---- scalar functionals (rank-0 forms): quadrature data reduced to numbers on the device ------------------------------
 * The reference's `fem.assemble_scalar`: J = g(u) * ds and f(u * u) * dx over a cell subset with their derivatives
 * (test/test_codim_external_operator.py), and the error norm sqrt(assemble_scalar((u - u_UFL)**2 * dx)) that ends
 * demo_hyperelasticity.py (:817). All array pointers are DEVICE pointers, 8-byte aligned (DXO_E_ALIGN otherwise; `cells` 4-byte)
 * and non-NULL where a length above zero makes them needed (DXO_E_NULL otherwise; `out` always). Asynchronous on the context's stream.
 * dxo_eval_cell_measure : dx[n_cells][nq] = w_q |det J|, the cell counterpart of dS (dxo_eval_facet_geometry). cells / n_cells as for
 *     dxo_eval_operand: an entity list (not range-checked), or NULL for the cells [0, n_cells) (n_cells < 0: all).
 * dxo_integrate : f [n_cells][nq][D], indexed by POSITION in the list — the layout Expression.eval / dxo_eval_operand write.
 *     g == NULL: out[k] = sum_c sum_q w_q |det J| f[c][q][k] for k < D, the integrals of the D components, for the value sizes this
 *                library's operators produce, D = 1, 2, 3, 4, 6, 9 (any other: DXO_E_DIM).
 *     g != NULL, shaped like f: out[0] = sum_c sum_q w_q |det J| sum_k f_k g_k, the pairing int f : g dx, any D in 1 .. 2^24
 *                (g == f is allowed: int |f|^2 dx).
 * dxo_facet_integrate : the same two forms over a facet set with dS, f [n][nq_facet][D]. The checks are dxo_facet_adjoint's: facet
 *     geometry not set DXO_E_OPTION; a set created on another mesh, or tables / geometry changed to another (nf, nq): DXO_E_DIM.
 * dxo_operand_moments : the fused form — the operand is formed from the dofs u in registers and never written:
 *     out[k] = int operand_k(u) dx for k < D, out[D] = int |operand(u)|^2 dx, D = dxo_operand_value_size(gdim, bs, kind), out D + 1
 *     doubles. Every kind dxo_eval_operand takes, at bs = 1 or gdim; other block sizes DXO_E_DIM (the per-component launches have
 *     no fused form), an unknown kind DXO_E_OPTION. VALUE: the mean of u and the squared L2 norm (of a difference field: the demo's
 *     error norm); GRAD: the squared H1 seminorm; DETF: the deformed volume; DIV: the net outflow.
 * The cell calls need dxo_mesh_set_weights (DXO_E_OPTION otherwise). |det J|, not det J: a mirrored mesh integrates to the same
 * value. A list may repeat a cell; it is then counted as often, as dxo_eval_operand evaluates it as often.
 * `out` is SET, never accumulated (option "consumer_overwrite" does not apply), and an empty list or set gives exactly +0.0 in every
 * entry: a functional over nothing is 0.
 * No atomics, bit-reproducible, and the bits do not depend on the launch shape or the device's compute-unit count: every GROUP — the
 * floor(64 / nq) consecutive cells of the list one wave takes, or floor(64 / nq_facet) consecutive entities (one for a rule of 64
 * points or more) — sums its points in a fixed lane order and writes one partial per output to a scratch [n_out][n_groups]; a second
 * kernel, one workgroup per output, adds the partials in a fixed order (lane t of 256 takes groups t, t + 256, ... ascending, then a
 * fixed LDS tree joins the lanes). The scratch is grow-only and owned by the mesh (cell calls) or the facet set (facet call): the
 * first call of a size allocates it; after that the calls allocate and synchronise nothing (capture-safe). A mesh whose vertices
 * and parked values exceed the 64 KiB LDS budget is refused with DXO_E_SIZE. */
int dxo_eval_cell_measure(dxo_ctx* ctx, dxo_mesh* mesh, const int32_t* cells, int64_t n_cells, double* dx);
int dxo_integrate(dxo_ctx* ctx, dxo_mesh* mesh, const int32_t* cells, int64_t n_cells, int D, const double* f, const double* g,
                  double* out);
int dxo_facet_integrate(dxo_ctx* ctx, dxo_mesh* mesh, dxo_facet_set* set, int D, const double* f, const double* g, double* out);
int dxo_operand_moments(dxo_ctx* ctx, dxo_mesh* mesh, int kind, int bs, const double* u, const int32_t* cells, int64_t n_cells,
                        double* out);

/* ---- coefficient assigners on the device, DEVICE memory only --------------------------
 * One scatter for the reference's three dofmap assigners (src/dolfinx_external_operator/external_operator.py):
 * _assign_non_mixed :286-287, _assign_mixed_2d :292-311, _assign_mixed_3d :313-335. For cell c, point p < n_pts,
 * component v < val_size:
 *   coeff[flat_dofs[(c*n_pts + p)*val_size + v]] = values[(c*n_points_total + offset + p)*comp_size + v]
 * Non-mixed: offset = 0, n_points_total = n_pts, comp_size = val_size and flat_dofs = the unrolled dofmap (:18-26);
 * mixed: one call per subspace with its offset / n_pts / val_size (:180-190) and the operator's comp_size (:161).
 * Where several entries target the same dof the LAST one (largest source position) wins, as in NumPy's sequential
 * fancy assignment, so the result is the reference's array, not a race. flat_dofs entries must lie in
 * [0, coeff_size): out-of-range entries are skipped on the device and the call returns DXO_E_SIZE (the NumPy
 * assigner raises IndexError, :287); the check costs one stream synchronisation per call, option
 * "assign_validate" = 0 skips it (entries are still never written out of bounds). The pass that finds the last writer
 * keeps one word per coefficient entry: 32-bit while the entry count is below 2^32 - 1, 64-bit beyond (option
 * "assign_owner_bits" = 64 takes the wide words at any size: the same result, for tests). */
typedef struct dxo_assign_desc {
    int64_t n_cells;
    int32_t n_pts, val_size, offset, n_points_total, comp_size;
    int32_t elem_bytes;     /* width of one scalar of `values` / `coeff`: 4 (float32), 8 (float64), 16 (complex128); 0 = 8. The
                               reference's assigners take whatever scalar type the function space has (float32 / float64 /
                               complex128 in test/test_multiaction.py:15-23): values are moved, never computed on. ABI version 2
                               (version 1 had padding here and moved 8-byte elements only) */
} dxo_assign_desc;
int dxo_assign(dxo_ctx* ctx, const dxo_assign_desc* desc, const int32_t* flat_dofs, const void* values,
               void* coeff, int64_t coeff_size);
/* The same assignment as a PLAN (round 4). Which entry wins a shared dof depends on the dofmap alone, and the dofmap of a
 * function space does not change between the calls of a solve (the reference builds its unrolled dofmaps once, in the
 * operator's constructor, external_operator.py:203-209): dxo_assign_plan_create runs the ownership pass once and keeps, per
 * coefficient entry, the position in `values` of the last entry that targets it; dxo_assign_apply is then ONE gather
 * (coeff[d] = values[src[d]] for the targeted entries, the others keep their value) with coalesced stores and no atomics —
 * bit-identical to dxo_assign at a fraction of its cost (0.60 -> 0.083 ms for 3.4*10^7 entries into 10^7 dofs,
 * profiles/r06_assign_sorted.txt). flat_dofs is device memory and is not kept; out-of-range entries make the creation fail with DXO_E_SIZE. */
typedef struct dxo_assign_plan dxo_assign_plan;
int dxo_assign_plan_create(dxo_ctx* ctx, const dxo_assign_desc* desc, const int32_t* flat_dofs, int64_t coeff_size,
                           dxo_assign_plan** out);
void dxo_assign_plan_destroy(dxo_ctx* ctx, dxo_assign_plan* plan);
int dxo_assign_apply(dxo_ctx* ctx, const dxo_assign_plan* plan, const void* values, void* coeff);   /* elements of the width the plan's descriptor named */
/* A plan of 2^20 coefficient entries or more carries the assignment in two orders (round 6): by coefficient entry (sequential stores, gathered
 * loads) and by position in `values` (near-sequential loads, scattered stores). Which is faster depends on how the caller's dofs are numbered
 * against its cells (Q2 hexahedra 108^3: 0.089 / 0.090 ms with one numbering, 0.107 / 0.085 with another, profiles/r06_assign_sorted.txt), so the
 * FIRST dxo_assign_apply of such a plan launches each form twice on the caller's arrays (every launch leaves the same coefficient), times the
 * second launches and keeps the faster form from then on; a call made while its stream is being captured takes the first form and decides
 * later. Option "assign_plan_form" at creation: 0 = as described, 1 = entry order only, 2 = source order (any size). Returns the form in use
 * (0 = not decided yet, 1, 2) and the two timings in ms (0 until measured); pointers may be NULL. */
int dxo_assign_plan_form(const dxo_assign_plan* plan, double* ms_dof_order, double* ms_source_order);

/* Operand evaluation FUSED in front of the heat-flux kernel: T and sigma = grad T of a scalar Lagrange field on
 * `mesh` are formed per quadrature point and fed to q_impl / dqdT_impl / dqdsigma_impl
 * (demo_nonlinear_heat_equation_part2.py:219-261) in the same launch. T_dofs: num_field_nodes doubles; outputs cover
 * all cells: q[n][gdim], dqdT[n][gdim], dqdsigma[n][gdim][gdim], n = num_cells*nq; any output may be NULL. */
int dxo_heat_field(dxo_ctx* ctx, double A, double B, dxo_mesh* mesh, int mem, const double* T_dofs,
                   double* q, double* dqdT, double* dqdsigma);

/* The Newton / network / analytic hyperelastic operators with the operand formed on the device from the dof vector of
 * the displacement field on `mesh` (gdim = 2): the reference's pair evaluate_operands + evaluate_external_operators
 * (demo_plasticity_mohr_coulomb.py:679-688, demo_hyperelasticity.py:548-557) behind one call.
 *   dxo_mohr_coulomb_field   operand eps(Du) in Mandel notation (:163-165), then dxo_mohr_coulomb's kernels; sigma_n and
 *                            the outputs cover all cells, n = num_cells*nq points, diagnostics as in dxo_mohr_coulomb
 *   dxo_icnn_field           operand F = I + grad u (demo_hyperelasticity.py:479), then dxo_icnn_eval's kernel
 *   dxo_isihara_field        the same operand in front of dxo_isihara
 * u: num_field_nodes*2 doubles (blocked, as fem.Function.x.array). A host caller uploads the dof vector instead of the
 * operand array. dxo_isihara_field (HBM-bound) forms F in the registers of the kernel that evaluates the model, F never
 * reaches memory; for the two compute-bound operators (fp64 Newton, fp32 MFMA network) the operand values pass through a
 * staging buffer of the context in HBM between the operand kernel and theirs (csrc/field_ops.hip). Results are
 * bit-identical to dxo_eval_operand followed by the plain entry point. */
int dxo_mohr_coulomb_field(dxo_ctx* ctx, const dxo_mc_params* prm, dxo_mesh* mesh, int mem, const double* u,
                           const double* sigma_n, double* C_tang, double* sigma, int32_t* niter, double* yielding,
                           double* norm_res, double* dlambda);
int dxo_icnn_field(dxo_ctx* ctx, const dxo_icnn* model, int precision, dxo_mesh* mesh, int mem, const double* u,
                   double* dP, double* P);
int dxo_isihara_field(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, int mem, const double* u,
                      double* dP, double* P);
/* dxo_mohr_coulomb3 with the operand formed on the device: eps(Du) of a gdim = 3 mesh (six Mandel components) into the
 * staging buffer, then dxo_mohr_coulomb3's kernels. u: num_field_nodes*3 doubles; sigma_n and the outputs cover all cells,
 * n = num_cells*nq points. Bit-identical to dxo_eval_operand followed by dxo_mohr_coulomb3. A mesh with gdim != 3: DXO_E_DIM. */
int dxo_mohr_coulomb3_field(dxo_ctx* ctx, const dxo_mc_params* prm, dxo_mesh* mesh, int mem, const double* u,
                            const double* sigma_n, double* C_tang, double* sigma, int32_t* niter, double* yielding,
                            double* norm_res, double* dlambda);

/* The analytic Isihara energy for a 3x3 deformation gradient, the full 3-D form of dxo_isihara's:
 *   W = c1 (I1bar-3) + c2 (I2bar-3) + c3 (I1bar-3)^2 + c4 (J-1)^2,  I1bar = J^(-2/3) I1, I2bar = J^(-4/3) I2,
 *   I1 = tr C, I2 = (I1^2 - tr C^2) / 2, C = F^T F, J = det F
 * (for F = [[F_2, 0], [0, 1]] its in-plane stress and tangent are dxo_isihara's). c3 = 0 is the compressible Mooney-Rivlin solid,
 * c2 = c3 = 0 the neo-Hookean one. F[n][9] row-major (F_ia at 3 i + a) -> dP[n][9][9] (dP_i/dF_j, symmetric: a Hessian), P[n][9],
 * fp64 throughout; det F <= 0 -> NaN in all 90 outputs of the point. dP is the [n][9][9] block of the ("grad", "grad", bs = 3)
 * bilinear pair and P the operand of the internal force. Checks and error codes as dxo_isihara; device arrays 16-byte aligned.
 *   dxo_isihara3_field   F = I + grad u formed in the registers of the same kernel from the dof vector u (num_field_nodes*3 doubles)
 *                        of a gdim = 3 mesh (DXO_E_DIM otherwise); any element dxo_mesh_create accepts. Checks as dxo_isihara_field. */
int dxo_isihara3(dxo_ctx* ctx, const dxo_isihara_params* prm, int64_t n, int mem,
                 const double* F, double* dP, double* P);
int dxo_isihara3_field(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, int mem, const double* u,
                       double* dP, double* P);
/* The three consumers of dxo_isihara3_field's outputs as functions of the dof vector u alone, WITHOUT the quadrature arrays: the model
 * has no history, so F = I + grad u, the stress and the tangent's action are formed again in the registers of every call (the action
 * dP/dF : grad v costs about 150 flops per point and never forms the 45-entry Hessian) and dP[n][9][9], P[n][9] (720 B per point) need
 * not exist. For a matrix-free Newton-Krylov solve on a gdim = 3 mesh, bs = 3:
 *   dxo_isihara3_residual          R   (+)= sum_q w|det J| B^T P(I + grad u)                  = dxo_isihara3_field + dxo_operand_adjoint("F")
 *   dxo_isihara3_tangent_apply     out (+)= sum_q w|det J| B^T (dP/dF(I + grad u) : grad v)  = ... + dxo_bilinear_apply(grad, grad, 3)
 *   dxo_isihara3_tangent_diagonal  the diagonal of the same operator                        = ... + dxo_bilinear_diagonal(grad, grad, 3)
 * to rounding (the contractions run in another order). Consumer semantics as dxo_bilinear_apply: DEVICE pointers only, u / v / R / out
 * num_field_nodes*3 doubles, out += (SET with option consumer_overwrite), two passes without atomics where the mesh allows them,
 * bit-reproducible, capture-safe; weights from dxo_mesh_set_weights. det F <= 0 at a point: NaN in every dof of its cell, as the array
 * route. DXO_E_NULL for a NULL params, mesh or array, DXO_E_DIM for gdim != 3, DXO_E_OPTION without weights, DXO_E_ALIGN for an array
 * not 8-byte aligned, DXO_E_SIZE for an element too large for the LDS budget (no mesh the array route accepts); num_cells == 0: DXO_OK. */
int dxo_isihara3_residual(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, double* R);
int dxo_isihara3_tangent_apply(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, const double* v,
                               double* out);
int dxo_isihara3_tangent_diagonal(dxo_ctx* ctx, const dxo_isihara_params* prm, dxo_mesh* mesh, const double* u, double* out);

/* The network operator for a 3x3 deformation gradient: the SAME dxo_icnn model (one weight set serves both dimensions) evaluated
 * on the invariants of the full C = F^T F,
 *   K1 = I1 I3^(-1/3) - 3,  K2 = I2 I3^(-2/3) - 3,  K3 = (sqrt(I3) - 1)^2,  I1 = tr C, I2 = (I1^2 - tr C^2) / 2, I3 = (det F)^2,
 * which the reference writes out for F = [[F_2, 0], [0, 1]] (demo_hyperelasticity.py:263-283): the in-plane stress and tangent of an
 * embedded plane-strain F are dxo_icnn_eval's (up to the correction, which differs in the last bits of zero), the out-of-plane shear
 * stresses are exactly 0 and P_33 is not. I/O as dxo_isihara3: F[n][9] row-major -> dP[n][9][9] (symmetric), P[n][9]; precision as
 * dxo_icnn_eval; kernels by "icnn_variant" as in 2-D (0, 1, 2), the default one's stores by "icnn3_store" (0 — the default — one
 * 648-byte row per lane, 1 staged through LDS in output order: measured slower, profiles/icnn3_bench.txt). det F < 0 is finite (sqrt(I3) = |det F|, as the reference), det F = 0
 * gives non-finite values in that point's outputs only.
 *   dxo_icnn3_correction  H9[9]: the stress correction H = -P_NN(F = I) of :362-381 (P += F H, dP_(ia)(jc) += d_ij H_ca). In 3-D it is a
 *                         multiple of the identity and analytically zero (K1, K2, K3 are stationary at F = I): rounding of create().
 *   dxo_icnn3_field       F = I + grad u of a gdim = 3 mesh (DXO_E_DIM otherwise) into the context's staging buffer, then the network
 *                         kernel: the two-launch form of dxo_icnn_field; bit-identical to dxo_eval_operand + dxo_icnn3_eval.
 * Checks and error codes as dxo_isihara3 / dxo_isihara3_field, plus DXO_E_OPTION for a precision other than 0 or 1. */
int dxo_icnn3_eval(dxo_ctx* ctx, const dxo_icnn* model, int precision, int64_t n, int mem,
                   const double* F, double* dP, double* P);
int dxo_icnn3_field(dxo_ctx* ctx, const dxo_icnn* model, int precision, dxo_mesh* mesh, int mem, const double* u,
                    double* dP, double* P);
int dxo_icnn3_correction(dxo_ctx* ctx, const dxo_icnn* model, double* H9);

/* ---- multi-GPU: cell-block sharding + RCCL all-gather inside the library (BASELINE north_star) ----
 * The reference splits only by MPI mesh partition and never gathers quadrature data
 * (src/dolfinx_external_operator/external_operator.py:365-371, 445). Here ONE coefficient vector's quadrature points
 * are split into `world` contiguous, equally sized cell blocks; rank r owns points [r*n_per_rank, (r+1)*n_per_rank).
 * Each GPU evaluates its block and writes straight into its slice of FULL-length output arrays
 * (world*n_per_rank points, device memory on that GPU); RCCL's in-place all-gather over xGMI then gives every GPU the
 * whole vector. All calls are asynchronous on the contexts' streams (dxo_mgpu_synchronize waits).
 *   dxo_mgpu_create       one process, n_dev GPUs (devices == NULL: 0..n_dev-1): a dxo_ctx and a communicator per
 *                         device (ncclCommInitAll); the pointer arrays of the calls below have n_dev entries.
 *   dxo_mgpu_create_rank  one process per GPU: rank 0 calls dxo_mgpu_unique_id, the caller broadcasts the
 *                         DXO_MGPU_ID_BYTES bytes (MPI_Bcast, torch.distributed, a file ...), every rank joins with
 *                         its own ctx; pointer arrays have ONE entry. Collective: all ranks must call.
 * RCCL is loaded at the first dxo_mgpu_* call (dlopen librccl.so.1): DXO_E_NODEVICE if it is absent; RCCL errors are
 * returned as 10000 + ncclResult_t with the text in dxo_mgpu_last_error.
 * gather: DXO_GATHER_NONE (outputs are block-length arrays, no exchange), DXO_GATHER_FULL (all-gather of C_tang,
 * sigma, dp: (d*d+d+1) doubles per point per peer), DXO_GATHER_COMPACT (the kernel writes (sigma, dp) only, those are
 * all-gathered, and EVERY block's tangent — the rank's own too — is rebuilt on each GPU with dxo_vm_expand_tangent:
 * 6.1x fewer link bytes at d = 6; all ranks run the same rebuild on the same gathered values, so the replicas are
 * bit-identical across ranks; they agree with DXO_GATHER_FULL's tangents to rounding, see dxo_vm_expand_tangent, and the
 * reference's NaN tangent at f_elastic == 0 is reproduced on every rank through the dp = -0.0 mark, which is cleared
 * before the call returns). n_per_rank must be even with a gather (16-byte aligned blocks); pad the last block as
 * sharding.CellBlockPartition does. Buffers handed to a collective must be hipMalloc memory: the group's contexts have
 * "placement_vmm" = 0 and the collectives return DXO_E_MEM for a pointer inside a chunk-backed arena block. */
#define DXO_MGPU_ID_BYTES 128
#define DXO_GATHER_NONE 0
#define DXO_GATHER_FULL 1
#define DXO_GATHER_COMPACT 2
/* DXO_GATHER_COMPACT with the exchange of (sigma, dp) as ONE group of ncclSend / ncclRecv pairs (every rank's block straight to
 * every peer: on a fully connected xGMI node each block travels on its own link at once) instead of RCCL's
 * all-gather — same arrays afterwards, bit for bit. dxo_mgpu_von_mises only. */
#define DXO_GATHER_COMPACT_DIRECT 3
/* ... and with the block cut into option "mgpu_chunks" (default 4) pieces on 64-point borders: the kernel of piece k + 1 runs
 * while piece k is on the links (the library's own exchange stream per device), and piece k's tangents are rebuilt while later
 * pieces still travel (SURVEY.md 8e iii). Same arrays afterwards, bit for bit. dxo_mgpu_von_mises only. */
#define DXO_GATHER_COMPACT_PIPELINED 4
typedef struct dxo_mgpu dxo_mgpu;
int dxo_mgpu_create(const int* devices, int n_dev, dxo_mgpu** out);
/* Contexts only, no communicator and no RCCL: for dxo_mgpu_von_mises_host, whose data path has no exchange step. The
 * collective entry points return DXO_E_OPTION on such a group. A device may be listed more than once. */
int dxo_mgpu_create_local(const int* devices, int n_dev, dxo_mgpu** out);
int dxo_mgpu_unique_id(void* id128);
int dxo_mgpu_create_rank(dxo_ctx* ctx, const void* id128, int rank, int world, dxo_mgpu** out);
int dxo_mgpu_destroy(dxo_mgpu* g);
int dxo_mgpu_size(const dxo_mgpu* g);                 /* ranks in the communicator                      */
int dxo_mgpu_local_count(const dxo_mgpu* g);          /* devices driven by this process                 */
int dxo_mgpu_rank(const dxo_mgpu* g, int i);          /* global rank of local device i                  */
dxo_ctx* dxo_mgpu_ctx(dxo_mgpu* g, int i);            /* its context (options, dxo_output_alloc, ...)   */
const char* dxo_mgpu_last_error(const dxo_mgpu* g);
int dxo_mgpu_synchronize(dxo_mgpu* g);
/* In-place all-gather of count_per_rank doubles per rank: buf[i] = full-length array on local device i whose own
 * block already sits at offset rank*count_per_rank. */
int dxo_mgpu_all_gather(dxo_mgpu* g, double* const* buf, int64_t count_per_rank);
/* dxo_von_mises on every local device + the exchange. deps/sigma_n/p[i]: block of local device i (n_per_rank points);
 * C_tang/sigma/dp[i]: full-length arrays on that device (block-length with DXO_GATHER_NONE). */
int dxo_mgpu_von_mises(dxo_mgpu* g, const dxo_vm_params* prm, int d, int64_t n_per_rank, int gather,
                       const double* const* deps, const double* const* sigma_n, const double* const* p,
                       double* const* C_tang, double* const* sigma, double* const* dp);

/* The other pointwise operators sharded the same way (every kernel of the path is a pointwise map): each
 * local device evaluates its cell block (n_per_rank points, the single-GPU entry point on device memory) into its slice of
 * the FULL-length outputs, then one in-place all-gather per requested output array. gather: DXO_GATHER_NONE (block-length
 * outputs, no exchange) or DXO_GATHER_FULL; DXO_GATHER_COMPACT is refused (DXO_E_OPTION): only the von Mises tangent is a
 * function of the other outputs. With a gather n_per_rank must be a multiple of 4. A NULL pointer ARRAY (niter, yielding,
 * ..., q, dqdT, dqdsigma) means the output is not requested. models[i] is the dxo_icnn created on dxo_mgpu_ctx(g, i). */
int dxo_mgpu_mohr_coulomb(dxo_mgpu* g, const dxo_mc_params* prm, int64_t n_per_rank, int gather, const double* const* deps,
                          const double* const* sigma_n, double* const* C_tang, double* const* sigma, int32_t* const* niter,
                          double* const* yielding, double* const* norm_res, double* const* dlambda);
int dxo_mgpu_icnn(dxo_mgpu* g, dxo_icnn* const* models, int precision, int64_t n_per_rank, int gather, const double* const* F,
                  double* const* dP, double* const* P);
int dxo_mgpu_isihara(dxo_mgpu* g, const dxo_isihara_params* prm, int64_t n_per_rank, int gather, const double* const* F,
                     double* const* dP, double* const* P);
int dxo_mgpu_heat(dxo_mgpu* g, double A, double B, int gdim, int64_t n_per_rank, int gather, const double* const* T,
                  const double* const* sigma, double* const* q, double* const* dqdT, double* const* dqdsigma);

/* HOST arrays of all n points sharded over the local devices, no collective: contiguous blocks (borders on 64-point
 * tiles), one dxo_von_mises(DXO_MEM_HOST) per device, concurrently, each over its own PCIe link; results land in the
 * caller's arrays. The NumPy path is PCIe-bound, so the links are what scales it. Works on any group (create,
 * create_local; with create_rank it is the single local device). Options are those of the local contexts (dxo_mgpu_ctx). */
int dxo_mgpu_von_mises_host(dxo_mgpu* g, const dxo_vm_params* prm, int d, int64_t n, const double* deps,
                            const double* sigma_n, const double* p, double* C_tang, double* sigma, double* dp);

/* ---- HBM stream probe (measurement aid, device memory only) --------------------------------
 * Moves data with no arithmetic in the read : write mix of a constitutive kernel, lane-linear 16-byte
 * accesses: n_tiles tiles, each 64 lanes x read_chunks 16-byte loads and 64 x write_chunks 16-byte
 * stores. Supported mixes (read, write): (13,43) von Mises d=6, (9,21) von Mises d=4, (8,20)
 * Mohr-Coulomb, (6,21) Mohr-Coulomb on six components, (3,8) heat, (1,1) and (4,4) plain copy. src needs n_tiles*read_chunks*1024 bytes, dst
 * n_tiles*write_chunks*1024 bytes. bench.py reports its GB/s beside the 8 TB/s spec peak. */
int dxo_stream_probe(dxo_ctx* ctx, int read_chunks, int write_chunks, int64_t n_tiles,
                     const void* src, void* dst);

#ifdef __cplusplus
}
#endif
#endif /* DXO_H */
