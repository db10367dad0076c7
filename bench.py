#!/usr/bin/env python3
"""bench.py — quadrature-points/s of the fused von Mises return-map + consistent tangent on MI355X.

One "step" = one pass of the hot path over one batch of synthetic quadrature data already resident in
HBM: the kernel behind `external_function((1,))(deps)` (dxo_von_mises, device pointers) and, for N > 1,
the RCCL all-gather that reassembles the flat coefficient vectors (BASELINE north_star).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--nqp POINTS_PER_GPU] [--d 6]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself: the parent
process spawns `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD before importing torch or
touching the GPU, relays rank 0's single JSON line and exits with the child's code (never an exec, never a restart of a
process that has initialised HIP).

Workload (named in config.workload): 3-D hex mesh, 8 quadrature points per cell (degree-2 rule), Mandel
d = 6, fp64; 1 250 000 cells = 10^7 quadrature points per GPU — the size BASELINE.json's north_star quotes
the >= 70 %-of-HBM-roofline target on (config 2's 10^6 points is 448 MB, of which the 104 MB of inputs stay
in the 256 MB Infinity Cache between steps; scripts/bench_extra.py reports it). Scaling is weak: with N > 1 every
rank owns its own cell block of 1.25*10^7 points (BASELINE config 3: 10^8 points over 8 GPUs).

A plain run measures the headline and nothing else: set-up, W warm-up steps, ONE batch of exactly K timed steps, the outputs of
the last step written with `--dump-outputs DIR`, one result line. Everything beside the headline runs with `--full` only: the
cpu_baseline leg, the live HBM-counter passes, the stream probe, the side figures (plain allocation, factory), end_to_end, the
`secondary` block, the output checks, the median of 5 batches, and at N > 1 the other gather modes of a fixed --gather-mode,
the separate roofline launches and libdxo's own RCCL cross-check.

stdout carries the contract line (rank 0): a BOUNDED extract (tools/bench_line.py, <= 6 000 bytes) of the full record, which goes
to `bench_full.json` beside this file. A plain run writes it once. With `--full` and one GPU the line is written as soon as the
timed region is over and again — a superset each time — when `cpu_baseline` + the live HBM-counter passes are in and when the
end_to_end / secondary legs are done (the full record then also goes to stderr); the LAST line is the result. Under
torch.distributed (N > 1) with `--full` the line is written once and repeated with `gather_check` (the verdict of libdxo's own
RCCL path, run after the result) filled in.
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import statistics
import sys
import threading
import time

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
BYTES_PER_QP = {4: 240, 6: 448}  # algorithmic fp64 traffic per point, SURVEY.md 8(d)
PROBE_MIX = {4: (9, 21), 6: (13, 43)}  # 16-byte chunks read / written per pair of points
DUMP_POINTS = 1 << 17  # --dump-outputs: points written at most (45 MB at d = 6)
DUMP_SEED = 5


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def dump_outputs(torch, out_dir, C_tang, sigma, dp, d):
    """--dump-outputs: (C_tang, sigma, dp) of the last timed step as float64 .npy files, (P, d, d), (P, d), (P,). P = every point when
    there are at most DUMP_POINTS, otherwise a sorted sample of DUMP_POINTS points drawn with DUMP_SEED: the same points in every run of
    the same size, so that two builds can be compared output for output."""
    import numpy as np

    n = dp.numel()
    out_dir = pathlib.Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    arrays = {"C_tang": C_tang.view(n, d, d), "sigma": sigma.view(n, d), "dp": dp.view(n)}
    if n > DUMP_POINTS:
        idx = np.sort(np.random.Generator(np.random.PCG64(DUMP_SEED)).choice(n, size=DUMP_POINTS, replace=False))
        idx_dev = torch.from_numpy(idx).to(dp.device)
        arrays = {k: a.index_select(0, idx_dev) for k, a in arrays.items()}
    for name, a in arrays.items():
        np.save(out_dir / f"{name}.npy", a.cpu().numpy().astype(np.float64, copy=False))


def synth_inputs(torch, n, d, seed, device):
    """deps ~ N(0, 3e-3) (Mandel shear x sqrt 2), sigma_n ~ N(0, 100), p = |N(0, 1e-3)|.
    All three live in ONE slab (13 doubles per point at d = 6) so the stream probe can read exactly the
    same memory the kernel reads."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    slab = torch.empty(n * (2 * d + 1), dtype=torch.float64, device=device)
    deps = slab[: n * d].view(n, d)
    sigma_n = slab[n * d: 2 * n * d].view(n, d)
    p = slab[2 * n * d:]
    deps.normal_(0.0, 3e-3, generator=g)
    deps[:, 3:] *= 2.0 ** 0.5
    sigma_n.normal_(0.0, 100.0, generator=g)
    p.normal_(0.0, 1e-3, generator=g)
    p.abs_()
    return slab, deps, sigma_n, p


def cpu_baseline(d, n_sample, budget_s=10.0):
    """Time the CPU oracle (oracle/dxo_oracle.c, a statement-by-statement port of the reference's Numba
    kernel, OpenMP over points) on this host's cores, on a bounded sample of the same distribution.
    Output arrays are allocated and touched once, outside the timed passes."""
    import numpy as np

    from oracle import load_oracle

    o = load_oracle()
    rng = np.random.Generator(np.random.PCG64(1))
    deps = rng.normal(0.0, 3e-3, size=(n_sample, d))
    deps[:, 3:] *= np.sqrt(2.0)
    sigma_n = rng.normal(0.0, 100.0, size=(n_sample, d))
    p = np.abs(rng.normal(0.0, 1e-3, size=n_sample))
    out = (np.zeros((n_sample, d, d)), np.zeros((n_sample, d)), np.zeros(n_sample))
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)

    def one_pass(nt):
        t0 = time.perf_counter()
        o.von_mises(deps, sigma_n, p, nthreads=nt, out=out)
        return n_sample / (time.perf_counter() - t0)

    # The visible core count can exceed what the container may actually run (cgroup quota): scan thread
    # counts and keep the fastest; `cores` reports the thread count actually used for the quoted value.
    one_pass(avail)  # thread-pool + page warm-up
    scan = {}
    nt = 1
    while nt <= avail:
        scan[nt] = max(one_pass(nt), one_pass(nt))
        nt *= 2
    if avail not in scan:
        scan[avail] = max(one_pass(avail), one_pass(avail))
    # the two best thread counts of the scan are then run SUSTAINED (half the budget each) and the better median is the figure: a count
    # that wins two short passes can lose over seconds (a cgroup quota throttles 128 spinning threads: one lease in ten read 20x low)
    best_two = sorted(scan, key=scan.get, reverse=True)[:2]
    sustained = {}
    for nt_ in best_two:
        rr, t_all = [], time.perf_counter()
        while len(rr) < 3 or (time.perf_counter() - t_all < budget_s / len(best_two) and len(rr) < 200):
            rr.append(one_pass(nt_))
        sustained[nt_] = rr
    threads = max(sustained, key=lambda k: statistics.median(sustained[k]))
    rates = sustained[threads]
    return {
        "value": statistics.median(rates), "unit": "qp/s", "cores": threads, "kind": "port",
        "sample": f"{n_sample} points x {len(rates)} passes (median of passes), d={d}, same input distribution; "
                  f"oracle/dxo_oracle.c (C port of the reference's Numba kernel) with OpenMP over points, "
                  f"fastest of thread counts {sorted(scan)} on {avail} visible cores (the two best of the scan run sustained, the better median kept)",
        "value_1core": scan[1], "thread_scan": {str(k): v for k, v in scan.items()},
    }


def measure_traffic(n, d, timeout_s=90):
    """HBM bytes per launch of the headline kernel from the PMC counters, measured NOW: two child runs of this script under
    `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes, counters only — MI355X_MICROARCH.md "HBM"), 3 timed
    steps each on the same workload (plain allocation: counters do not depend on placement). bytes = counter x 1024, and
    FETCH_SIZE doubled (on gfx950 it reports half of a wide coalesced streaming read). Returns (bytes per launch, detail) or
    (None, why). The children are separate processes started with subprocess (never an exec of this process)."""
    import csv
    import shutil
    import subprocess
    import tempfile

    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not pathlib.Path(prof).exists():
        return None, "rocprofv3 not found"
    grid = (n + 255) // 256 * 256
    got = {}
    for counter, corr in (("FETCH_SIZE", 2.0), ("WRITE_SIZE", 1.0)):
        with tempfile.TemporaryDirectory(prefix="dxo_pmc_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
            cmd = [prof, "--pmc", counter, "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, str(pathlib.Path(__file__).resolve()),
                   "--steps", "3", "--warmup", "1", "--batches", "1", "--nqp", str(n), "--d", str(d), "--placement", "0", "--no-cpu", "--no-probe", "--no-e2e",
                   "--no-secondary", "--no-traffic", "--no-side"]
            try:
                res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout_s, cwd=tmp)
            except (subprocess.TimeoutExpired, OSError) as exc:
                return None, f"{counter} pass: {exc!r}"
            vals = []
            for f in pathlib.Path(tmp).rglob("*counter_collection.csv"):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        if row.get("Counter_Name") == counter and "vm_tile<" in row.get("Kernel_Name", "") and int(row.get("Grid_Size", 0)) == grid:
                            vals.append(float(row["Counter_Value"]))
            if not vals:
                return None, f"{counter} pass: no vm_tile dispatch of grid {grid} in the counter file (rc {res.returncode})"
            got[counter] = (sum(vals) / len(vals) * 1024.0 * corr, len(vals))
    total = got["FETCH_SIZE"][0] + got["WRITE_SIZE"][0]
    return total, {"fetch_bytes": got["FETCH_SIZE"][0], "write_bytes": got["WRITE_SIZE"][0], "launches_averaged": got["FETCH_SIZE"][1],
                   "method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE, separate child runs of bench.py made by this run; bytes = counter*1024, "
                             "FETCH_SIZE x2 (gfx950 wide-stream under-count, MI355X_MICROARCH.md)"}


def end_to_end(ctx, prm, d, sizes=(1_000_000, 10_000_000), calls=3):
    """The drop-in boundary as the reference uses it — NumPy in, NumPy out (external_operator.py:432-446,
    demo_plasticity_von_mises.py:343-352): dxo_von_mises with DXO_MEM_HOST on page-locked host arrays, i.e.
    H2D + kernel + D2H through the chunked three-stream pipeline. Two forms of the D2H leg:
      copy     (C_tang, sigma, dp) come back over PCIe: 344 B/point at d = 6, bit-identical to a device call
      rebuild  only (sigma, dp) cross PCIe (56 B/point); the caller's C_tang array is rebuilt from them by the
               context's host threads while later chunks are in flight (option vm_host_tangent = 1)
      resident rebuild + the history variables sigma_n, p in a device mirror (dxo_vm_state, uploaded once before the
               timed calls: they change only at the end of a load step, demo_plasticity_von_mises.py:564-565, while
               every Newton iteration in between calls the operator): 48 B/point up, 56 B/point down
    Reported beside the headline, never as `value`. Times are medians over `calls` calls; h2d/kernel/d2h are sums
    of the per-chunk event times (they overlap, so they do not add up to total_ms)."""
    import numpy as np

    from dolfinx_external_operator_amd import MEM_HOST

    out = {"memory": "hipHostMalloc (page-locked) host arrays", "host_threads": ctx.get_option("host_threads"), "sizes": []}
    rng = np.random.Generator(np.random.PCG64(7))
    for n in sizes:
        bufs = [ctx.pinned_empty(m) for m in (n * d, n * d, n, n * d * d, n * d, n)]
        deps, sigma_n, p, C_tang, sigma, dp = bufs
        blk = min(n, 1_000_000)    # one seeded block of 10^6 points, repeated: the path is pointwise, so repetition is immaterial
        reps = -(-n // blk)
        deps[:] = np.tile(rng.normal(0.0, 3e-3, size=blk * d), reps)[: n * d]
        sigma_n[:] = np.tile(rng.normal(0.0, 100.0, size=blk * d), reps)[: n * d]
        p[:] = np.tile(np.abs(rng.normal(0.0, 1e-3, size=blk)), reps)[:n]
        entry = {"points": n}
        ref_C = None
        for mode, name in ((0, "copy"), (1, "rebuild")):
            ctx.set_option("vm_host_tangent", mode)
            rows = []
            for _ in range(calls + 1):
                t0 = time.perf_counter()
                ctx.von_mises(prm, d, n, MEM_HOST, deps, sigma_n, p, C_tang, sigma, dp)
                wall = time.perf_counter() - t0
                rows.append((wall, ctx.last_timing()))
            rows = sorted(rows[1:], key=lambda r: r[0])
            wall, t = rows[len(rows) // 2]
            entry[name] = {"qp_per_s": n / wall, "total_ms": wall * 1e3, "h2d_ms": t["h2d_ms"], "kernel_ms": t["kernel_ms"],
                           "d2h_ms": t["d2h_ms"], "pcie_bytes_per_qp": 8 * (2 * d + 1) + (8 * (d * d + d + 1) if mode == 0 else 8 * (d + 1))}
            if mode == 0:
                ref_C = C_tang[: 4096 * d * d].copy()
            else:   # the host-rebuilt tangent must agree with the one the device wrote
                err = float(np.max(np.abs(C_tang[: 4096 * d * d] - ref_C)) / np.max(np.abs(ref_C)))
                entry["rebuild_vs_copy_max_rel_err"] = err
                if not err < 1e-12:
                    raise SystemExit(f"bench: host-rebuilt tangent differs from the device tangent ({err:.2e})")
        ref_s, ref_dp, ref_C = sigma[: 4096 * d].copy(), dp[:4096].copy(), C_tang[: 4096 * d * d].copy()
        st = ctx.vm_state(d, n)
        t0 = time.perf_counter()
        st.upload(sigma_n, p)
        upload_ms = (time.perf_counter() - t0) * 1e3
        rows = []
        for _ in range(calls + 1):
            t0 = time.perf_counter()
            st.call(prm, MEM_HOST, deps, C_tang, sigma, dp)
            wall = time.perf_counter() - t0
            rows.append((wall, ctx.last_timing()))
        rows = sorted(rows[1:], key=lambda r: r[0])
        wall, t = rows[len(rows) // 2]
        entry["resident"] = {"qp_per_s": n / wall, "total_ms": wall * 1e3, "h2d_ms": t["h2d_ms"], "kernel_ms": t["kernel_ms"],
                             "d2h_ms": t["d2h_ms"], "pcie_bytes_per_qp": 8 * d + 8 * (d + 1), "state_upload_once_ms": upload_ms}
        st.close()
        if not (np.array_equal(sigma[: 4096 * d], ref_s) and np.array_equal(dp[:4096], ref_dp) and np.array_equal(C_tang[: 4096 * d * d], ref_C)):
            raise SystemExit("bench: the resident-state call differs from the plain host call")
        ctx.set_option("vm_host_tangent", 0)
        if n == sizes[-1]:
            entry["through_dispatcher"] = through_dispatcher(ctx, n, d, deps, sigma_n, p)
        for b in bufs:
            ctx.pinned_free(b)
        out["sizes"].append(entry)
    return out


def through_dispatcher(ctx, n, d, deps, sigma_n, p, nq=8, calls=3):
    """One level above the C ABI: the factory called the way the reference calls it, through the value-side mirror of
    evaluate_external_operators (external_operator.py:407-448), which ends with `coefficient.x.array[:] = values` (:289-290)
    — a 36 N-double single-threaded host copy unless the factory was given the coefficient as its output (`outputs=`:
    the assignment is then array-to-itself, which NumPy skips). ms per call, median."""
    import numpy as np

    from dolfinx_external_operator_amd import QuadratureExternalOperator, evaluate_external_operators, evaluate_operands, make_von_mises
    from dolfinx_external_operator_amd.evaluation import Operand

    nc = n // nq
    operand = Operand(lambda cells: deps.reshape(nc, nq, d), "deps")
    res = {"points": n, "unit": "ms per evaluate_external_operators call",
           "meaning": {"default": "make_von_mises(sigma_n, p): the dispatcher copies the 36 N doubles into the coefficient (external_operator.py:441)",
                       "bind": "the one-line configuration, make_von_mises(sigma_n, p).bind(operator): results land in the coefficient's own storage",
                       "bind_resident_state": "bind + state='resident' (history variables mirrored on the device)"}}
    for label, kw, with_out in (("default", {}, False), ("bind", {}, True), ("bind_resident_state", {"state": "resident"}, True)):
        op = QuadratureExternalOperator(operand, num_cells=nc, num_points=nq, value_shape=(d, d), derivatives=(1,))
        op.external_function = make_von_mises(sigma_n, p, ctx=ctx, **kw)
        if with_out:
            op.external_function.bind(op)
        ts = []
        for _ in range(calls + 1):
            ev = evaluate_operands([op])
            t0 = time.perf_counter()
            evaluate_external_operators([op], ev)
            ts.append(time.perf_counter() - t0)
        res[label] = round(statistics.median(ts[1:]) * 1e3, 2)
        res.setdefault("calls_ms", {})[label] = [round(t * 1e3, 1) for t in ts]      # the first is the warm-up (first touch of the coefficient's pages)
        del op
    return res


def library_gather_check(torch, dist, ctx, prm, d, rank, world, device, n=1 << 20, steps=5, n_full=0, steps_full=0):
    """After the result line is out: the same split + exchange through the C ABI's own RCCL path (dxo_mgpu_create_rank /
    dxo_mgpu_von_mises, csrc/mgpu.hip) on a small batch, compared with torch.distributed's all-gather of the same
    blocks. Reported on stderr only; the result line is already out when it starts. A collective that does not come back
    ends the process with exit code 3 (a rank that has touched the GPU and gives up must not report success)."""
    import threading

    from dolfinx_external_operator_amd import GATHER_COMPACT, GATHER_COMPACT_DIRECT, GATHER_COMPACT_PIPELINED, GATHER_FULL, MultiGpu

    done = threading.Event()

    def watchdog():
        if not done.wait(170.0):
            log(f"bench rank {rank}: library_gather_check did not finish in 170 s — leaving with exit code 3 (the result line is already out)")
            os._exit(3)

    threading.Thread(target=watchdog, daemon=True).start()
    uid = [MultiGpu.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(uid, src=0)
    mg = MultiGpu.from_rank(ctx, uid[0], rank, world)
    g = torch.Generator(device=device)
    g.manual_seed(1000 + rank)
    deps = torch.empty(n, d, dtype=torch.float64, device=device).normal_(0.0, 3e-3, generator=g)
    sigma_n = torch.empty(n, d, dtype=torch.float64, device=device).normal_(0.0, 100.0, generator=g)
    p = torch.empty(n, dtype=torch.float64, device=device).normal_(0.0, 1e-3, generator=g).abs_()
    out = {}
    for mode, name in ((GATHER_FULL, "full"), (GATHER_COMPACT, "compact"), (GATHER_COMPACT_DIRECT, "direct"), (GATHER_COMPACT_PIPELINED, "pipelined")):
        C = torch.zeros(world * n * d * d, dtype=torch.float64, device=device)
        s = torch.zeros(world * n * d, dtype=torch.float64, device=device)
        dp = torch.zeros(world * n, dtype=torch.float64, device=device)
        mg.von_mises(prm, d, n, mode, [deps], [sigma_n], [p], [C], [s], [dp])
        mg.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            mg.von_mises(prm, d, n, mode, [deps], [sigma_n], [p], [C], [s], [dp])
        mg.synchronize()
        out[name] = {"ms_per_step": (time.perf_counter() - t0) / steps * 1e3, "C": C, "s": s, "dp": dp}
    # reference: every rank's own block through torch.distributed
    own = slice(rank * n * d, (rank + 1) * n * d)
    s_ref = torch.empty_like(out["full"]["s"])
    dist.all_gather_into_tensor(s_ref, out["full"]["s"][own].clone())
    err_s = float((out["full"]["s"] - s_ref).abs().max())
    err_cs = float((out["compact"]["s"] - s_ref).abs().max())
    scale = float(out["full"]["C"].abs().max())
    err_C = float((out["compact"]["C"] - out["full"]["C"]).abs().max()) / scale      # rebuilt tangents vs gathered ones
    # compact replicas must be the same BYTES on every rank (every rank rebuilds every block from the same gathered state)
    chk = torch.stack([out["compact"]["C"].view(torch.int64).sum(), out["compact"]["dp"].view(torch.int64).sum()])
    lo, hi = chk.clone(), chk.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    identical = bool((lo == hi).all())
    # the direct and the pipelined form leave the SAME arrays as compact, bit for bit (NaN-safe: compared as integers)
    same_forms = all(bool(torch.equal(out[k]["C"].view(torch.int64), out["compact"]["C"].view(torch.int64))) and
                     bool(torch.equal(out[k]["s"], out["compact"]["s"])) and bool(torch.equal(out[k]["dp"].view(torch.int64), out["compact"]["dp"].view(torch.int64)))
                     for k in ("direct", "pipelined"))
    # the same forms at the bench's own size (what `config.gather_modes` reports for the torch.distributed side): K steps each,
    # one set of full-length arrays; times are this rank's, rank 0 reports the maximum over ranks
    full_size = None
    if n_full > 0 and steps_full > 0:
        del C, s, dp
        for v in out.values():
            v.pop("C"), v.pop("s"), v.pop("dp")
        torch.cuda.empty_cache()
        g.manual_seed(100 + rank)
        deps = torch.empty(n_full, d, dtype=torch.float64, device=device).normal_(0.0, 3e-3, generator=g)
        sigma_n = torch.empty(n_full, d, dtype=torch.float64, device=device).normal_(0.0, 100.0, generator=g)
        p = torch.empty(n_full, dtype=torch.float64, device=device).normal_(0.0, 1e-3, generator=g).abs_()
        C = torch.empty(world * n_full * d * d, dtype=torch.float64, device=device)
        s = torch.empty(world * n_full * d, dtype=torch.float64, device=device)
        dp = torch.empty(world * n_full, dtype=torch.float64, device=device)
        times = []
        names = (("compact", GATHER_COMPACT), ("direct", GATHER_COMPACT_DIRECT), ("pipelined", GATHER_COMPACT_PIPELINED), ("full", GATHER_FULL))
        for name, mode in names:
            mg.von_mises(prm, d, n_full, mode, [deps], [sigma_n], [p], [C], [s], [dp])
            mg.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(steps_full):
                mg.von_mises(prm, d, n_full, mode, [deps], [sigma_n], [p], [C], [s], [dp])
            mg.synchronize()
            times.append((time.perf_counter() - t0) / steps_full * 1e3)
        tt = torch.tensor(times, dtype=torch.float64, device=device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        full_size = {"points_per_rank": n_full, "steps": steps_full, **{name: float(tt[i]) for i, (name, _) in enumerate(names)}}
    mg.close()
    done.set()
    ok = err_s == 0.0 and err_cs == 0.0 and err_C < 1e-13 and identical and same_forms
    rec = {"library_gather_check": "ok" if ok else "MISMATCH", "rank": rank, "rccl_ranks_in_libdxo": world, "points_per_rank": n,
           "full_ms_per_step": out["full"]["ms_per_step"], "compact_ms_per_step": out["compact"]["ms_per_step"],
           "direct_ms_per_step": out["direct"]["ms_per_step"], "overlap_ms_per_step": out["pipelined"]["ms_per_step"],
           "sigma_vs_torch_all_gather_max_abs": err_s, "compact_vs_full_tangent_max_rel": err_C,
           "compact_replicas_bit_identical": identical, "direct_and_pipelined_equal_compact_bitwise": same_forms,
           "library_full_size_ms_per_step": full_size}
    log(json.dumps(rec))
    return rec


def launch_ranks(n_gpus: int, argv: list[str]) -> int:
    """Parent side of `python bench.py --gpus N` (N > 1): one rank per GPU under torch.distributed.run, started as a
    child process. This function runs BEFORE torch is imported and makes no HIP / torch.cuda call, so the parent never
    initialises the GPU; the ranks check the device count themselves and fail loudly if the node has fewer GPUs."""
    import socket
    import subprocess

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sock:   # a free rendezvous port on the loopback
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: the only form this pool's host driver supports
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(pathlib.Path(__file__).resolve()), *argv]
    log("bench: launching", " ".join(cmd))
    res = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)   # stderr passes through
    lines = [ln for ln in res.stdout.decode(errors="replace").splitlines() if ln.strip()]
    json_lines = [ln for ln in lines if ln.lstrip().startswith("{")]
    for ln in lines:
        if ln not in json_lines:
            log(ln)
    if json_lines:
        print(json_lines[-1], flush=True)   # also the `"degraded": true` line of a run that then gave up on a hung collective
    if res.returncode != 0 or not json_lines:
        log(f"bench: the {n_gpus}-rank run failed (exit code {res.returncode}, {len(json_lines)} result lines)")
        return res.returncode or 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline (see the module docstring); a plain run times exactly --steps steps "
                         "and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/C_tang.npy, sigma.npy, dp.npy (float64; rank 0's arrays): "
                         f"all points up to {DUMP_POINTS}, above that the same seeded sample of {DUMP_POINTS} points in every run")
    ap.add_argument("--batches", type=int, default=None,
                    help="timed batches of --steps steps each, every batch between its own fences; value / ms_per_step are the median batch's "
                         "(SURVEY.md 8d timing protocol). Default 1, 5 with --full")
    ap.add_argument("--nqp", type=int, default=0,
                    help="quadrature points per GPU; default 10^7 at --gpus 1 (north_star's target size) and 1.25*10^7 at "
                         "--gpus N > 1 (BASELINE config 3: 10^8 points over 8 GPUs)")
    ap.add_argument("--d", type=int, default=6, choices=(4, 6))
    ap.add_argument("--nq", type=int, default=8, help="points per cell (bookkeeping only)")
    ap.add_argument("--gather", type=int, default=-1, help="all-gather outputs each step: -1 auto (N>1), 0, 1")
    ap.add_argument("--gather-mode", choices=("auto", "compact", "compact_pipelined", "compact_direct", "full"), default="auto",
                    help="compact: RCCL all-gather of (sigma, dp) + local rebuild of the remote tangents "
                         "(dxo_vm_expand_tangent); compact_pipelined: the same in 4 pieces, rebuild overlapped with the "
                         "link traffic; compact_direct: (sigma, dp) exchanged as one batch of RCCL sends / receives, every "
                         "block on its own xGMI link; full: RCCL all-gather of (C_tang, sigma, dp). Every mode is timed over the same K "
                         "steps and reported under config.gather_modes; auto (default) makes the fastest of them the headline "
                         "(all three leave the same arrays on every rank) and names it in config.gather.")
    ap.add_argument("--dry-collective", action="store_true",
                    help="logic check of the N > 1 path on a box with ONE GPU: all ranks share device 0 and the collectives "
                         "run over gloo instead of RCCL (RCCL refuses two ranks on one device). The line it prints is marked "
                         "`dry_collective` and is not a measurement.")
    ap.add_argument("--no-library-gather", action="store_true",
                    help="skip the dxo_mgpu_* (RCCL inside libdxo_hip.so) cross-check that runs after the result line at N > 1")
    ap.add_argument("--gather-vmm", type=int, default=0,
                    help="1: let the gathered (RCCL send / receive) arrays live in a virtual range backed by 2 MB chunks too "
                         "(experiment; default 0 = hipMalloc candidates only, see the comment at placement_vmm below); sets "
                         "DXO_ALLOW_VMM_COLLECTIVE=1 on every rank, without which sharding.py refuses such buffers; libdxo's own "
                         "forms (the cross-check after the line) refuse them always")
    ap.add_argument("--no-side", action="store_true",
                    help="skip the side figures measured after the timed batches (plain-allocation and factory launches of the same kernel): "
                         "profiled runs use it so that the LAST batches x steps dispatches of the headline kernel are the timed ones")
    ap.add_argument("--no-cpu", action="store_true", help="skip the cpu_baseline leg")
    ap.add_argument("--no-probe", action="store_true", help="skip the no-arithmetic stream probe")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end_to_end (H2D + kernel + D2H) leg")
    ap.add_argument("--no-traffic", action="store_true",
                    help="skip the live HBM-counter measurement (two short child runs under rocprofv3 --pmc); roofline.traffic is then null")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the `secondary` block (BASELINE configs 4 and 5, the reference's d = 4 layout, the fused operand + "
                         "return-map kernel: tools/bench_secondary.py)")
    ap.add_argument("--secondary-points", type=int, default=10_000_000)
    ap.add_argument("--secondary-budget", type=float, default=90.0,
                    help="seconds of wall the secondary legs (and their counter passes) may use: a leg that would start after the deadline is skipped and "
                         "named in secondary.skipped (the default run must finish well inside the driver's patience)")
    ap.add_argument("--cpu-budget", type=float, default=8.0, help="seconds of timed passes of the headline's cpu_baseline leg")
    ap.add_argument("--variant", type=int, default=1)
    ap.add_argument("--nontemporal", type=int, default=-1)
    ap.add_argument("--blocks-per-cu", type=int, default=-1)
    ap.add_argument("--placement", type=int, default=16,
                    help="candidates of the LIBRARY's output-arena calibration (ctx option placement_candidates; "
                         "0/1 = plain hipMalloc). The bench itself selects nothing. See DESIGN.md 3.1.")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if not args.full:   # a plain run: the headline alone
        args.no_cpu = args.no_probe = args.no_e2e = args.no_traffic = args.no_secondary = args.no_side = args.no_library_gather = True
    if args.gather_vmm:
        # the experiment this flag names hands chunk-backed arena blocks to the collectives, which sharding.py refuses by default
        # (set here, before anything is imported, and inherited by the ranks a parent launches); libdxo's own forms refuse such
        # buffers regardless (DXO_E_MEM), so the library cross-check after the line reports an error in this configuration
        os.environ["DXO_ALLOW_VMM_COLLECTIVE"] = "1"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))

    # stdout carries nothing but result lines (see the module docstring). Libraries that write to fd 1 on their own (RCCL prints a version
    # banner when its first communicator comes up) are sent to stderr: fd 1 is pointed at fd 2 for the whole run and
    # the JSON line is written to a saved copy of the real stdout at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"WORLD_SIZE={world} but --gpus {args.gpus}")
    n_dev = torch.cuda.device_count()   # counting devices does not initialise HIP
    if args.dry_collective:
        local_rank = 0
    if n_dev < (1 if args.dry_collective else max(world, 1)) or local_rank >= n_dev:
        raise SystemExit(f"bench.py rank {rank}: --gpus {args.gpus} needs {world} MI355X on this node, {n_dev} visible. "
                         "There is no CPU path to benchmark (only the cpu_baseline leg uses the oracle).")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    # under torch.distributed.run the process group is always brought up (also for a single rank, which
    # lets the RCCL path be exercised on a 1-GPU box with --gather 1)
    dist_on = world > 1 or "TORCHELASTIC_RUN_ID" in os.environ
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dry_collective:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)  # RCCL over xGMI

    from dolfinx_external_operator_amd import MEM_DEVICE, Context, VmParams
    from dolfinx_external_operator_amd._build import build_library
    from dolfinx_external_operator_amd.sharding import (WAVE_TILE, all_gather_in_place, gather_von_mises_compact,
                                                        gather_von_mises_compact_direct, gather_von_mises_compact_pipelined,
                                                        in_place_status)

    if rank == 0:
        build_library()
    if dist_on:
        dist.barrier()

    d, K, W = args.d, args.steps, args.warmup
    nqp = args.nqp if args.nqp > 0 else (10_000_000 if world == 1 else 12_500_000)
    n = (nqp + 2 * WAVE_TILE - 1) // (2 * WAVE_TILE) * (2 * WAVE_TILE)  # shard borders on wave tiles
    gather = (world > 1) if args.gather < 0 else bool(args.gather)
    E, nu, sigma_0 = 70e3, 0.3, 250.0
    H = E * (E / 100.0) / (E - E / 100.0)
    prm = VmParams(E, nu, sigma_0, H)

    ctx = Context(local_rank)
    info = ctx.device_info()
    ctx.set_option("vm_variant", args.variant)
    if args.nontemporal >= 0:
        ctx.set_option("nontemporal", args.nontemporal)
    if args.blocks_per_cu >= 0:
        ctx.set_option("blocks_per_cu", args.blocks_per_cu)
    stream = torch.cuda.current_stream(device)
    ctx.set_stream(stream.cuda_stream)

    seed = 1 if world == 1 else 100 + rank
    in_slab, deps, sigma_n, p = synth_inputs(torch, n, d, seed, device)
    # Outputs live in the library's OUTPUT ARENA (dxo_output_alloc, csrc/arena.hip): on this chip the rate of a multi-GB
    # streaming-write sweep depends on the allocation it goes to, so the library makes a few ordinary
    # allocations side by side, times a write sweep on each and keeps the fastest. This is what any user of
    # `Context.output_tensors` / `make_von_mises(...).arena(n, d)` gets; the bench does no selection of its own any
    # more. `roofline.achieved_plain_hipMalloc` is the same kernel writing into a plain torch.empty slab.
    # With the gather on, every rank holds the FULL-length outputs and its kernel writes its cell block straight
    # into them at [rank*n, (rank+1)*n): the all-gather is RCCL's in-place form and nothing is copied locally.
    gather_on = gather and dist_on
    blocks = world if gather_on else 1
    own = rank if gather_on else 0
    per_pt = d * d + d + 1
    N_full = blocks * n
    if args.placement <= 1:
        ctx.set_option("placement_mode", 0)
    else:
        ctx.set_option("placement_candidates", args.placement)   # the library caps it so that all candidates fit 60 % of the free memory
        ctx.set_option("placement_mode", 2)
        if gather_on and not args.gather_vmm:
            # the gathered arrays are RCCL send / receive buffers: plain hipMalloc blocks only (a virtual range backed by
            # 2 MB chunks cannot be exported with hipIpcGetMemHandle, which RCCL may use for peer access)
            ctx.set_option("placement_vmm", 0)
        elif gather_on and args.gather_vmm >= 2:
            ctx.set_option("placement_vmm", 2)   # chunk-backed candidates only
    # what make_von_mises(...).arena(n, d) hands out: candidates timed with the kernel itself, block and launch shape
    # (dxo_vm_output_alloc); with the gather on, the block holds the FULL-length arrays (hipMalloc candidates only, see above)
    C_full, sigma_full, dp_full = ctx.vm_output_tensors(N_full, d)
    placement = dict(C_full.dxo_block.info)
    C_tang = C_full[own * n * d * d:(own + 1) * n * d * d]
    sigma = sigma_full[own * n * d:(own + 1) * n * d]
    dp = dp_full[own * n:(own + 1) * n]

    plain_GBps = factory_GBps = factory_fresh_GBps = factory_placement = factory_detail = None      # side figures, filled in after the timed batches

    def bytes_per_launch_of(d_, n_):
        return BYTES_PER_QP[d_] * n_

    def time_kernel(out_ptrs, launches):
        pp = (deps.data_ptr(), sigma_n.data_ptr(), p.data_ptr(), *out_ptrs)
        ctx.von_mises(prm, d, n, MEM_DEVICE, *pp)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):   # back to back: a single isolated launch reads ~7 % faster than the sustained rate
            ctx.von_mises(prm, d, n, MEM_DEVICE, *pp)
        e1.record(stream)
        torch.cuda.synchronize(device)
        return BYTES_PER_QP[d] * n / (e0.elapsed_time(e1) / launches * 1e-3) / 1e9

    ptrs = (deps.data_ptr(), sigma_n.data_ptr(), p.data_ptr(), C_tang.data_ptr(), sigma.data_ptr(), dp.data_ptr())

    def expand(s_view, dp_view, C_view, npts):
        ctx.vm_expand_tangent(prm, d, npts, MEM_DEVICE, s_view.data_ptr(), dp_view.data_ptr(), C_view.data_ptr())

    def clear_marks(dp_view, npts):
        ctx.vm_clear_marks(npts, dp_view.data_ptr())

    # the compact forms: the kernel writes (sigma, dp) only (C_tang = NULL) with the reference's 0/0 point marked in the sign
    # bit of dp, (sigma, dp) go over the links, every rank rebuilds EVERY block's tangent (its own too: bit-identical
    # replicas, NaN at the marked points like the reference) and clears the marks
    ptrs_state_only = (*ptrs[:3], None, ptrs[4], ptrs[5])
    rebuild = dict(identical=True, clear_marks=clear_marks)

    def make_step(mode):
        compact = gather_on and mode.startswith("compact")
        def step(ev=None):
            if ev is not None:
                ev[0].record(stream)
            if compact:
                ctx.set_option("vm_mark_indeterminate", 1)
                ctx.von_mises(prm, d, n, MEM_DEVICE, *ptrs_state_only)
                ctx.set_option("vm_mark_indeterminate", 0)
            else:
                ctx.von_mises(prm, d, n, MEM_DEVICE, *ptrs)
            if ev is not None:
                ev[1].record(stream)
            if not gather_on:
                return
            if mode == "compact":
                gather_von_mises_compact(C_full, sigma_full, dp_full, rank, d, expand, **rebuild)
            elif mode == "compact_pipelined":
                gather_von_mises_compact_pipelined(C_full, sigma_full, dp_full, rank, d, expand, chunks=4, **rebuild)
            elif mode == "compact_direct":
                gather_von_mises_compact_direct(C_full, sigma_full, dp_full, rank, d, expand, **rebuild)
            else:
                for buf in (C_full, sigma_full, dp_full):
                    all_gather_in_place(buf, rank)
        return step

    auto_mode = args.gather_mode == "auto"
    if auto_mode:
        args.gather_mode = "compact"      # timed first; the others follow with the same protocol
    step = make_step(args.gather_mode)

    def fence():
        torch.cuda.synchronize(device)
        if dist_on:
            dist.barrier()
            torch.cuda.synchronize(device)

    # Timing protocol: W warm-up steps, then B batches of EXACTLY K steps, each batch between its own
    # pair of fences (synchronize + barrier + synchronize); `value` / `ms_per_step` are the MEDIAN batch's (under torch.distributed
    # every batch time is first reduced with MAX over ranks). Every launch sits between two HIP events on the launch stream, so a
    # batch whose wall time and kernel time disagree shows where the time went: `step_gap_us_max` is the largest interval between
    # the end of one step's launch and the start of the next one's. Nothing is allocated or freed between warm-up and the last batch,
    # Python's collector is off, and the events already exist (an event is created by its first record).
    B = max(1, args.batches if args.batches is not None else (5 if args.full else 1))
    import gc

    def run_batches(step_fn, warm):
        """`warm` untimed steps, then B batches of K steps; returns this rank's batch wall times, the mean kernel-event time of every
        batch and the step gaps (microseconds) of every batch."""
        for _ in range(warm):
            step_fn()
        evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)] for _ in range(B)]
        for batch in evs:
            for e_pair in batch:
                e_pair[0].record(stream)
                e_pair[1].record(stream)
        gc.collect()
        gc.disable()
        try:
            walls = []
            for b_ in range(B):
                fence()
                t0 = time.perf_counter()
                for k in range(K):
                    step_fn(evs[b_][k])
                fence()
                walls.append(time.perf_counter() - t0)
        finally:
            gc.enable()
        kern = [sum(a.elapsed_time(e) for a, e in batch) / K for batch in evs]
        gaps = [[batch[k][1].elapsed_time(batch[k + 1][0]) * 1e3 for k in range(K - 1)] for batch in evs]
        return walls, kern, gaps

    from tools.bench_timing import batch_record as _batch_record

    def batch_record(walls, kern, gaps):
        """The median batch and what the line says about all of them (tools/bench_timing.py; walls: already the maximum over ranks)."""
        return _batch_record(walls, kern, gaps, K, gather_on)

    def reduce_walls(walls):
        if not dist_on:     # one batch time for the job = the slowest rank's
            return list(walls)
        tb = torch.tensor(walls, dtype=torch.float64, device=device)
        dist.all_reduce(tb, op=dist.ReduceOp.MAX)
        return [float(x) for x in tb]

    walls, kernel_ms_batches, step_gaps_us = run_batches(step, W)
    walls = reduce_walls(walls)
    b_med, batch_stats = batch_record(walls, kernel_ms_batches, step_gaps_us)
    elapsed = walls[b_med]
    kernel_ms_avg = kernel_ms_batches[b_med]
    if gather_on:
        # in the compact forms the step's own launch is the (sigma, dp)-only kernel; `roofline` and `kernel_only_value` are
        # about the FULL kernel (448 B/point), so with a gather on it is timed here, K launches back to back into this
        # rank's slice of the same arrays (outside the timed steps; the next step overwrites the slice anyway). A plain run
        # leaves them out (null).
        kernel_ms_avg = bytes_per_launch_of(d, n) / time_kernel(ptrs[3:], K) / 1e6 if args.full else None
    total_points = n * world
    bytes_per_launch = BYTES_PER_QP[d] * n
    MODES = ("compact", "compact_pipelined", "compact_direct", "full")
    emitted = threading.Lock()
    last_result = {}

    def write_line(result, stage):
        """Rank 0: the bounded contract line (tools/bench_line.py, <= 6 000 bytes) to the real stdout; the full record to
        bench_full.json beside this file (and, at the final stage, to stderr)."""
        from tools.bench_line import compact_line

        os.write(real_stdout, (compact_line(result, stage) + "\n").encode())
        try:
            (ROOT / "bench_full.json").write_text(json.dumps({**result, "line": stage}) + "\n")
        except OSError as exc:
            log(f"bench: bench_full.json not written: {exc!r}")

    def emit_result(elapsed_, kernel_ms_, other_, probe_GBps=None, note=None, extras=True, degraded=False, mode=None, stats=None):
        """Rank 0: build the result and write its line to the real stdout. With one GPU the line is written THREE times, each a
        complete contract line and each a superset of the one before: (1) `headline` as soon as the timed region is over,
        (2) `headline+cpu`, then `headline+cpu+traffic` once the CPU port / the live HBM-counter passes are in, (3) `final` = the same with one
        short record per end_to_end / secondary leg. A reader takes the last line; a run cut short still leaves a valid one."""
        if rank != 0 or not emitted.acquire(blocking=False):
            return
        mode = mode or args.gather_mode
        achieved = bytes_per_launch / (kernel_ms_ * 1e-3) / 1e9 if kernel_ms_ is not None else None
        result = {
            "metric": "quadrature-points/sec (von Mises return-map + tangent)",
            "value": total_points * K / elapsed_, "unit": "qp/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": elapsed_ / K * 1e3, "higher_is_better": True, "scaling": "weak",
            "timing": {"protocol": f"{W} warm-up steps, then {B} batches of {K} steps, each batch between its own fences (synchronize + barrier); "
                                   "value and ms_per_step are the median batch's (max over ranks per batch); HIP events around every launch",
                       **{k: v for k, v in (stats or {}).items() if k not in ("batches", "ms_per_step_batches", "kernel_ms_batches", "step_gap_us_max")}},
            **{k: (stats or {}).get(k) for k in ("batches", "ms_per_step_batches", "kernel_ms_batches", "step_gap_us_max")},
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            **({"dry_collective": "NOT A MEASUREMENT: all ranks on one GPU, gloo collectives (logic check of the N > 1 path)"}
               if args.dry_collective else {}),
            **({"degraded": True} if degraded else {}),
            **({"note": note} if note else {}),
            "config": {
                "workload": f"von Mises radial return + consistent tangent, 3-D hex mesh, {args.nq} qp/cell, Mandel d={d}, "
                            f"{n // args.nq} cells = {n} quadrature points per GPU, fp64"
                            + ((", cell-block sharded, RCCL exchange of (sigma, dp) + on-device rebuild of the remote "
                                "tangents every step" if mode.startswith("compact") else
                                ", cell-block sharded, RCCL all-gather of (C_tang, sigma, dp) every step") if gather_on
                               else (", cell-block sharded, no gather" if world > 1 else "")),
                "points_per_gpu": n, "cells_per_gpu": n // args.nq, "nq": args.nq, "d": d,
                "sharding": "cell-block" if world > 1 else "none",
                "gather": f"rccl_all_gather_{mode}" if gather_on else "none",
                "gather_mode_selection": ("auto: the fastest of the timed modes is the headline" if auto_mode else "fixed by --gather-mode") if gather_on else None,
                "gather_modes": ({m: {"value": total_points * K / t_m, "ms_per_step": t_m / K * 1e3,
                                      "link_bytes_per_qp": 8 * per_pt if m == "full" else 8 * (d + 1),
                                      **({"ms_per_step_batches": other_stats[m]["ms_per_step_batches"]} if m in other_stats else {})}
                                  for m, t_m in {mode: elapsed_, **other_}.items()} if gather_on else None),
                "gather_modes_meaning": ({"full": "north_star's plain RCCL all-gather of all three output arrays",
                                          "compact": "kernel writes (sigma, dp) only; all-gather of (sigma, dp); every rank rebuilds EVERY block's "
                                                     "tangent (replicas bit-identical across ranks, equal to the full form's to rounding; the "
                                                     "reference's NaN tangent at f_el == 0 carried by the sign bit of dp, cleared afterwards)",
                                          "compact_pipelined": "compact in 4 pieces, rebuild overlapped with the link traffic",
                                          "compact_direct": "compact with (sigma, dp) exchanged as ONE batch of point-to-point sends / receives "
                                                            "(every block on its own xGMI link at once) instead of the library's all-gather",
                                          "library forms": "libdxo's own RCCL path (dxo_mgpu_von_mises, what a C / MPI caller gets) is timed at this "
                                                           "size AFTER this line is out and reported under gather_check.library_full_size_ms_per_step; "
                                                           "it is never the headline"}
                                         if gather_on else None),
                "rccl_ranks": world if dist_on else 0,
                "collective_backend": (dist.get_backend() if dist_on else None),
                # what sharding.all_gather_in_place was told to do (decided before any rank issues a collective)
                "gather_in_place": (in_place_status() if gather_on else None),
                "mode_status": ({m: ("timed" if (m == mode or m in other_) else "failed or skipped: see stderr") for m in MODES} if gather_on else None),
                "placement_candidates_requested": args.placement, "placement_candidates_probed": placement.get("candidates"),
                "placement_block_bytes": N_full * per_pt * 8,
                "kernel": "vm_tile" if args.variant else "vm_point",
                "arch": info["arch"], "compute_units": info["compute_units"],
            },
            "roofline": {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS if achieved is not None else None, "traffic": None, "traffic_detail": None,
                "traffic_over_algorithmic": None,
                "kernel": f"vm_tile<{d}>" if args.variant else f"vm_point<{d}>",
                "kernel_ms_avg": kernel_ms_, "algorithmic_bytes_per_launch": bytes_per_launch,
                "bytes_per_qp": BYTES_PER_QP[d],
                "output_memory": "dxo_output_alloc (library output arena, " + placement["mode"] + ")",
                "placement": placement,
                "achieved_plain_hipMalloc": plain_GBps,
                "achieved_factory_device_call_arena_outputs": factory_GBps,
                "achieved_factory_default_device_call": factory_fresh_GBps,
                "factory_placement": factory_placement, "factory_detail": factory_detail,
                "stream_probe_GBps": probe_GBps,
            },
            "kernel_only_value": total_points / (kernel_ms_ * 1e-3) if kernel_ms_ is not None else None,
        }
        if dist_on:
            result["gather_check"] = ({"status": "skipped", "why": "dry_collective: libdxo's own RCCL path needs one GPU per rank"} if args.dry_collective
                                      else {"status": "skipped", "why": "--no-library-gather" if args.full else "runs with --full"} if args.no_library_gather
                                      else {"status": "pending", "why": "runs after this line; a second, final line repeats this one with the verdict"})
        last_result.update(result)
        # a plain run, and under torch.distributed (also a world of one) every run: the line is written once (with --full under
        # torch.distributed, then once more with gather_check)
        single = extras and world == 1 and not dist_on and args.full
        t_extras = time.perf_counter()
        if not single:
            write_line(result, "final")
            return
        write_line(result, "headline")      # (1) the contract line exists from here on
        # first the CPU port's timed passes (host cores only, nothing else of this run active), THEN the live HBM-counter passes (two
        # child runs of this script under rocprofv3 --pmc: Python + torch imports, input generation — they would take cores and memory
        # bandwidth from the CPU figure if they ran beside it)
        if not args.no_cpu:
            try:
                result["cpu_baseline"] = cpu_baseline(d, 2_000_000, budget_s=args.cpu_budget)
            except Exception as exc:   # noqa: BLE001
                log(f"bench: cpu_baseline failed: {exc!r}")
            write_line(result, "headline+cpu")
        if not args.no_traffic:
            try:
                traffic, traffic_detail = measure_traffic(n, d)      # each child under its own timeout; nothing runs on after it
            except Exception as exc:   # noqa: BLE001 — a side leg must never cost the line
                traffic, traffic_detail = None, repr(exc)
            result["roofline"].update(traffic=traffic, traffic_detail=traffic_detail,
                                      traffic_over_algorithmic=(traffic / bytes_per_launch) if traffic else None)
        write_line(result, "headline+cpu+traffic")      # (2)
        result["wall_s"] = {"cpu_and_traffic": round(time.perf_counter() - t_extras, 1)}
        if not args.no_e2e:
            t_leg = time.perf_counter()
            try:
                result["end_to_end"] = end_to_end(ctx, prm, d)
            except SystemExit:
                raise
            except Exception as exc:   # noqa: BLE001
                log(f"bench: end_to_end failed: {exc!r}")
            result["wall_s"]["end_to_end"] = round(time.perf_counter() - t_leg, 1)
        if not args.no_secondary:
            # the other BASELINE configs, each with its own roofline and cpu_baseline (never `value`)
            t_leg = time.perf_counter()
            try:
                from tools.bench_secondary import secondary_block

                result["secondary"] = secondary_block(torch, ctx, stream, prm, n=args.secondary_points, cpu=not args.no_cpu,
                                                      deadline=time.perf_counter() + args.secondary_budget)
            except Exception as exc:   # noqa: BLE001
                log(f"bench: secondary block failed: {exc!r}")
            result["wall_s"]["secondary"] = round(time.perf_counter() - t_leg, 1)
        last_result.update(result)
        log(json.dumps(result))      # the full record: stderr + bench_full.json
        write_line(result, "final")      # (3)

    def emit_gather_check(rec):
        """Rank 0: the second, final line = the first with the verdict of the library's own RCCL path."""
        if rank != 0 or not last_result:
            return
        last_result["gather_check"] = rec
        write_line(last_result, "final+gather_check")

    # the other gather modes, same protocol, reported beside the headline (never as `value`). They are comparison figures:
    # if one of them — or the reduction of the times behind them — does not come back (a collective that hangs), rank 0
    # prints the line with the headline mode alone, from its own clock, marked `"degraded": true`, and every rank leaves
    # with exit code 3: a process that has touched the GPU and gives up on a hung collective must not report success.
    compare_done = threading.Event()
    other_elapsed, other_stats = {}, {}
    if gather_on and world > 1:
        def _compare_watchdog(elapsed_=elapsed, kernel_ms_=kernel_ms_avg, mode_=args.gather_mode, stats_=batch_stats):
            # headline time and mode captured by value before the comparison loop (the main thread reassigns them later)
            if not compare_done.wait(300.0):
                log(f"bench rank {rank}: the comparison gather modes did not come back in 300 s — reporting the headline mode alone, exit code 3")
                emit_result(elapsed_, kernel_ms_, {}, note="comparison gather modes abandoned after 300 s", extras=False, degraded=True, mode=mode_,
                            stats=stats_)
                os._exit(3)
        threading.Thread(target=_compare_watchdog, daemon=True).start()
    if gather_on and (auto_mode or args.full):      # a plain run with a fixed --gather-mode times that mode alone
        if world > 1 and args.full:   # remote tangents rebuilt from (sigma, dp) must be usable: finite and symmetric
            nb = (rank + 1) % world
            chk = C_full[nb * n * d * d: nb * n * d * d + 4096 * d * d].view(-1, d, d)
            if not bool(torch.isfinite(chk).all()) or float((chk - chk.transpose(1, 2)).abs().max()) > 1e-9 * E:
                raise SystemExit("bench: gathered/rebuilt remote C_tang block is not a finite symmetric tangent")
        sums = (float(sigma_full.sum()), float(dp_full.sum()))      # every mode must leave the same gathered arrays
        # Every form is a sequence of torch.distributed collectives that all ranks enter alike: nothing below can fail on one rank
        # and not on the others except the collective itself, and a raise out of a collective is FATAL (sharding.py) — there is no
        # per-mode try: a rank that skipped a mode its peers had entered would leave them waiting in it. (libdxo's own RCCL forms,
        # whose communicator bootstrap CAN fail locally, are timed after the result line is out: library_gather_check.)
        for mode in MODES:
            if mode == args.gather_mode:
                continue
            w2, k2, g2 = run_batches(make_step(mode), min(W, 2))
            if (float(sigma_full.sum()), float(dp_full.sum())) != sums:
                raise SystemExit(f"bench: gather mode '{mode}' left different (sigma, dp) than the headline mode")
            w2 = reduce_walls(w2)
            bm, st = batch_record(w2, k2, g2)
            other_elapsed[mode], other_stats[mode] = w2[bm], st

    if dist_on:
        kernel_ms_avg_max = None
        if kernel_ms_avg is not None:
            t = torch.tensor([kernel_ms_avg], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            kernel_ms_avg_max = float(t[0])
        if auto_mode and gather_on:
            # the reduced times are identical on every rank, so every rank picks the same headline
            best = min({args.gather_mode: elapsed, **other_elapsed}.items(), key=lambda kv: kv[1])
            if best[0] != args.gather_mode:
                other_elapsed[args.gather_mode], other_stats[args.gather_mode] = elapsed, batch_stats
                args.gather_mode, elapsed = best
                del other_elapsed[args.gather_mode]
                batch_stats = other_stats.pop(args.gather_mode)
    else:
        kernel_ms_avg_max = kernel_ms_avg
    compare_done.set()

    # what the caller of the timed path receives after its last step: the full-length arrays with the gather on, else this rank's own
    if args.dump_outputs and rank == 0:
        dump_outputs(torch, args.dump_outputs, *((C_full, sigma_full, dp_full) if gather_on else (C_tang, sigma, dp)), d)

    # correctness tripwire inside the bench itself (not timed, --full): plastic points sit on the yield surface — checked on
    # the first and on the LAST 4096 points (the tail exercises the 64-bit index arithmetic of very large batches)
    for lo in sorted({0, max(n - 4096, 0)}) if args.full else ():
        sl = slice(lo, lo + 4096)
        s_chk = sigma.view(n, d)[sl]
        dev_chk = s_chk.clone()
        dev_chk[:, :3] -= s_chk[:, :3].mean(dim=1, keepdim=True)
        f_chk = (1.5 * (dev_chk * dev_chk).sum(1)).sqrt() - sigma_0 - H * (p[sl] + dp[sl])
        plastic = dp[sl] > 0
        if plastic.any() and float(f_chk[plastic].abs().max()) > 1e-8 * sigma_0:
            raise SystemExit("bench: yield condition violated by the kernel output — refusing to report a number")
        if not bool(torch.isfinite(C_tang[lo * d * d:(lo + 4096) * d * d]).all()):
            raise SystemExit("bench: non-finite tangent in the kernel output — refusing to report a number")
        del s_chk, dev_chk, f_chk, plastic      # s_chk is a view into the headline's output block: it must not outlive the block's release below

    # side figures (never `value`), measured AFTER the timed batches so that their allocations and frees cannot disturb them
    if rank == 0 and not gather_on and not args.no_side:
        plain = torch.empty(n * per_pt, dtype=torch.float64, device=device)   # what an un-placed allocation gives
        plain_GBps = time_kernel((plain.data_ptr(), plain.data_ptr() + n * d * d * 8, plain.data_ptr() + n * (d * d + d) * 8), 12)
        del plain
        torch.cuda.empty_cache()

    # stream probe: a no-arithmetic kernel moving the same read:write mix (13 : 43 sixteen-byte rows per tile) from the
    # input slab into the SAME output block, persistent grid of 16 workgroups per CU. A reference point beside the
    # 8 TB/s spec peak — NOT a ceiling: its access pattern differs from the kernel's (one output stream, not three).
    probe_GBps = None
    if rank == 0 and not args.no_probe:
        R, Wc = PROBE_MIX[d]
        tiles = n // (2 * WAVE_TILE)
        saved_bpc = ctx.get_option("blocks_per_cu")
        ctx.set_option("blocks_per_cu", 16)
        for _ in range(W):
            ctx.stream_probe(R, Wc, tiles, in_slab.data_ptr(), C_full.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(K):
            ctx.stream_probe(R, Wc, tiles, in_slab.data_ptr(), C_full.data_ptr())
        e1.record(stream)
        torch.cuda.synchronize(device)
        ctx.set_option("blocks_per_cu", saved_bpc)
        probe_GBps = tiles * (R + Wc) * 1024 / (e0.elapsed_time(e1) / K * 1e-3) / 1e9

    # The factory leg below is what a USER of make_von_mises gets, and a user does not hold a second 3.4 GB output block: the headline's block goes
    # back to the context first (dxo_output_free keeps one calibrated block for the next request of its size, csrc/arena.hip — on a box with ONE
    # fast range among 68 candidates, round 6 lease 14, nothing else could give the factory the headline's rate), and the factory's own
    # calibration is then handed that block (factory_placement.rounds == 0) or searches afresh.
    released_headline_block = False
    if rank == 0 and world == 1 and not dist_on and not gather_on and not args.no_side:
        del C_tang, sigma, dp, C_full, sigma_full, dp_full
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        released_headline_block = True

    # the same kernel through the drop-in factory with CUDA-tensor operands, make_von_mises(...)((1,))(deps): with its DEFAULTS
    # (fresh output tensors at every call, the reference's semantics) and with the one-keyword opt-in device_outputs="arena"
    # (outputs in a persistent arena block of the operator's own, overwritten by its next call)
    if rank == 0 and not gather_on and not args.no_side and n * per_pt * 8 >= ctx.get_option("placement_min_bytes") and 3 * n * per_pt * 8 < info["total_mem_bytes"] // 4:
        from dolfinx_external_operator_amd import make_von_mises

        deps3 = deps.view(n // args.nq, args.nq, d)
        rates = []
        factory_detail = {}
        for kw in ({"device_outputs": "arena"}, {}):
            ext = make_von_mises(sigma_n, p, E=E, nu=nu, sigma_0=sigma_0, H=H, ctx=ctx, **kw)
            f = ext((1,))
            res_ = f(deps3)
            blk_ = getattr(res_[0], "dxo_block", None)
            if blk_ is not None and kw:
                factory_placement = {k: blk_.info.get(k) for k in ("mode", "candidates", "chosen_kind", "chosen_GBps", "rounds", "calibration_ms")}
                factory_placement["block"] = ("the headline's block, handed back by the context's cache (rounds = 0)" if blk_.info.get("rounds") == 0
                                              else "its own search" + (", made after the headline's block was released" if released_headline_block else ""))
            reps = []
            for _ in range(3):      # three runs of 12 launches: a transient (host hiccup) shows as one low run, a slow block as three
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(12):
                    f(deps3)
                e1.record(stream)
                torch.cuda.synchronize(device)
                reps.append(BYTES_PER_QP[d] * n / (e0.elapsed_time(e1) / 12 * 1e-3) / 1e9)
            rates.append(statistics.median(reps))
            factory_detail["arena" if kw else "fresh"] = {"runs_GBps": reps}
            if blk_ is not None and kw:
                # the same block through the thin entry point (no factory code between the launches): separates the block from the path
                factory_detail["arena"]["direct_entry_point_GBps"] = time_kernel(tuple(t.data_ptr() for t in res_), 12)
            del ext, f, res_, blk_
            torch.cuda.empty_cache()
        factory_GBps, factory_fresh_GBps = rates


    if rank == 0:
        if world == 1 and not args.no_e2e:
            if not released_headline_block:
                del C_tang, sigma, dp, C_full, sigma_full, dp_full
            del in_slab, deps, sigma_n, p
            torch.cuda.empty_cache()
        emit_result(elapsed, kernel_ms_avg_max, other_elapsed, probe_GBps, stats=batch_stats)
    if dist_on:
        # the result line is out; whatever is still running 180 s from now (a collective of the cross-check or the final
        # barrier that does not come back) is abandoned — with exit code 3, so that a hang is never recorded as success
        def _leave():
            time.sleep(180.0)
            log(f"bench rank {rank}: post-result phase still running after 180 s — leaving with exit code 3")
            os._exit(3)

        threading.Thread(target=_leave, daemon=True).start()
    if dist_on and not args.dry_collective and not args.no_library_gather:
        try:    # evidence for dxo_mgpu_* with more than one rank; stderr only, after the result line
            C_tang = sigma = dp = C_full = sigma_full = dp_full = None
            torch.cuda.empty_cache()
            rec = library_gather_check(torch, dist, ctx, prm, d, rank, world, device, n_full=n if gather_on else 0, steps_full=K)
            emit_gather_check({"status": rec["library_gather_check"], **{k: v for k, v in rec.items() if k not in ("library_gather_check", "rank")}})
        except Exception as exc:   # noqa: BLE001
            log(f"bench rank {rank}: library_gather_check failed: {exc!r}")
            emit_gather_check({"status": "error", "why": repr(exc)})
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
