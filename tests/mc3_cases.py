"""Shared helpers of the 3-D Mohr-Coulomb tests: seeded rotations, the orthogonal Mandel rotation R(Q), the plane-strain
embedding, the yield function evaluated from the 3x3 tensor in NumPy, and the g++ builds of the two test aids
(tests/helpers/mc3_core_cpu.cpp: host build of csrc/mc3_core.h; tests/helpers/mc3_referee.cpp: the reference's algorithm on six
components with dual numbers). Nothing here is shipped."""
import ctypes as C
import pathlib
import subprocess

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "dolfinx_external_operator_amd" / "csrc"
R2 = np.sqrt(2.0)


def rotations(n, seed):
    """n proper rotations (n,3,3), Haar-distributed: QR of a Gaussian matrix, signs fixed, det = +1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    A = rng.normal(size=(n, 3, 3))
    Q, Rr = np.linalg.qr(A)
    Q = Q * np.sign(np.einsum("nii->ni", Rr))[:, None, :]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def to_tensor(v):
    """Mandel (..., 6) -> symmetric (..., 3, 3)."""
    v = np.asarray(v, dtype=float)
    T = np.empty(v.shape[:-1] + (3, 3))
    T[..., 0, 0], T[..., 1, 1], T[..., 2, 2] = v[..., 0], v[..., 1], v[..., 2]
    T[..., 0, 1] = T[..., 1, 0] = v[..., 3] / R2
    T[..., 0, 2] = T[..., 2, 0] = v[..., 4] / R2
    T[..., 1, 2] = T[..., 2, 1] = v[..., 5] / R2
    return T


def to_mandel(T):
    T = np.asarray(T, dtype=float)
    return np.stack([T[..., 0, 0], T[..., 1, 1], T[..., 2, 2], R2 * T[..., 0, 1], R2 * T[..., 0, 2], R2 * T[..., 1, 2]], axis=-1)


def mandel_rotation(Q):
    """R(Q) (n,6,6) with mandel(Q A Q^T) = R(Q) mandel(A); orthogonal because the Mandel map is an isometry."""
    Q = np.asarray(Q, dtype=float).reshape(-1, 3, 3)
    R = np.empty((Q.shape[0], 6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1.0
        R[:, :, k] = to_mandel(Q @ to_tensor(e) @ np.swapaxes(Q, 1, 2))
    return R


def embed(v4):
    """Plane-strain (n,4) Mandel vector or (n,4,4) matrix -> six components, zeros in the out-of-plane shears."""
    v4 = np.asarray(v4, dtype=float)
    if v4.ndim == 2:
        out = np.zeros((v4.shape[0], 6))
        out[:, :4] = v4
        return out
    out = np.zeros((v4.shape[0], 6, 6))
    out[:, :4, :4] = v4
    return out


def rotate_vec(R, v):
    return np.einsum("nij,nj->ni", R, v)


def rotate_mat(R, M):
    return np.einsum("nij,njk,nlk->nil", R, M, R)


def _defaults():
    from oracle.loader import MC_DEFAULTS as D

    d = dict(D)
    if d["a"] is None:
        d["a"] = 0.26 * d["c"] / np.tan(d["phi"])
    return d


def surface_np(sig6, angle=None, **params):
    """The Abbo-Sloan surface at `angle` (default phi: the yield function f) from the 3x3 tensor: J2 = tr(s^2)/2, J3 = det s."""
    p = _defaults()
    p.update(params)
    angle = p["phi"] if angle is None else angle
    T = to_tensor(sig6)
    I1 = np.einsum("nii->n", T)
    s = T - I1[:, None, None] / 3.0 * np.eye(3)
    J2 = 0.5 * np.einsum("nij,nji->n", s, s)
    J3 = np.linalg.det(s)
    arg = np.clip(-(3.0 * np.sqrt(3.0) * J3) / (2.0 * np.sqrt(J2 ** 3)), -1.0, 1.0)
    th = np.arcsin(arg) / 3.0
    tT = p["theta_T"]
    sg = np.where(th < 0.0, -1.0, 1.0)
    k = np.sin(angle) / np.sqrt(3.0)
    c1 = np.cos(tT) - k * np.sin(tT)
    c2 = sg * np.sin(tT) + k * np.cos(tT)
    c3 = 18.0 * np.cos(3 * tT) ** 3
    Cc = (-np.cos(3 * tT) * c1 - 3.0 * sg * np.sin(3 * tT) * c2) / c3
    Bc = (sg * np.sin(6 * tT) * c1 - 6.0 * np.cos(6 * tT) * c2) / c3
    Ac = -k * sg * np.sin(tT) - Bc * sg * np.sin(3 * tT) - Cc * np.sin(3 * tT) ** 2 + np.cos(tT)
    K = np.where(np.abs(th) > tT, Ac + Bc * np.sin(3 * th) + Cc * np.sin(3 * th) ** 2, np.cos(th) - k * np.sin(th))
    ag = p["a"] * np.tan(p["phi"]) / np.tan(angle)
    return I1 / 3.0 * np.sin(angle) + np.sqrt(J2 * K * K + ag * ag * np.sin(angle) ** 2) - p["c"] * np.cos(angle)


def c_elas6():
    from tools.mc_inputs import MC_E, MC_NU

    lm = MC_E * MC_NU / ((1 + MC_NU) * (1 - 2 * MC_NU))
    mu = MC_E / (2 * (1 + MC_NU))
    Cel = 2 * mu * np.eye(6)
    Cel[:3, :3] += lm
    return Cel


def _runner(fn):
    def run(deps, sn, nthreads=1, **kw):
        from oracle.loader import mc_params

        prm = mc_params(**kw)
        deps = np.ascontiguousarray(deps, dtype=np.float64).reshape(-1, 6)
        sn = np.ascontiguousarray(sn, dtype=np.float64).reshape(-1, 6)
        n = len(deps)
        Ct, s = np.empty((n, 6, 6)), np.empty((n, 6))
        it, y, nr, dl = np.empty(n, dtype=np.int32), np.empty(n), np.empty(n), np.empty(n)
        args = [C.byref(prm), C.c_int64(n)] + [C.c_void_p(a.ctypes.data) for a in (deps, sn, Ct, s, it, y, nr, dl)]
        if nthreads is not None:
            args.append(C.c_int(int(nthreads)))
        fn(*args)
        return Ct, s, it, y, nr, dl

    return run


def build_aids(outdir):
    """Build both test aids with g++ into `outdir`; returns (lane, referee, referee_ld, lane_lib)."""
    outdir = pathlib.Path(outdir)
    core = outdir / "mc3_core_cpu.so"
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}",
                    str(ROOT / "tests" / "helpers" / "mc3_core_cpu.cpp"), "-o", str(core)], check=True)
    ref = outdir / "mc3_referee.so"
    subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-fopenmp", str(ROOT / "tests" / "helpers" / "mc3_referee.cpp"),
                    "-o", str(ref)], check=True)
    lc, lr = C.CDLL(str(core)), C.CDLL(str(ref))
    lane = _runner(lc.mc3_core_cpu)
    lane_run = lambda deps, sn, **kw: lane(deps, sn, nthreads=None, **kw)   # noqa: E731
    return lane_run, _runner(lr.mc3_referee), _runner(lr.mc3_referee_ld), lc


# ---- the cases and bounds the CPU and GPU tests share
# Bounds on |C_tang - referee| / max|C_tang| and |sigma - referee| / max(|sigma|, 1) on points with equal iteration counts: ten times
# the worst error of the host lane math against the long-double referee, measured by tests/test_mohr_coulomb3_cpu.py on the cases below
# (the measured figures stand in the docstrings there), and never looser than mc_compare's 1e-9.
BOUND_C_ROTATED = 1.8e-13   # measured 1.4e-14 (seed 2), 1.8e-14 (seed 5, shear 0.3)
BOUND_S_ROTATED = 2.4e-14   # measured 2.4e-15, 2.0e-15
BOUND_C_GENERAL = 1.1e-13   # measured 1.1e-14 (phi == psi), 1.8e-15 (phi != psi)
BOUND_S_GENERAL = 1.7e-14   # measured 1.7e-15, 5.7e-16

NON_ASSOCIATED = {"phi": 25 * np.pi / 180, "psi": 10 * np.pi / 180, "theta_T": 20 * np.pi / 180}


def general_states(n, seed=31, scale=1.0):
    """deps and sigma_n that share no principal axis: n points of the frozen tracing pool, each tensor turned by a rotation of its own."""
    from tools.mc_inputs import mc_pool

    pool_d, pool_s = mc_pool()
    rng = np.random.Generator(np.random.PCG64(seed))
    idx = rng.integers(0, pool_d.shape[0], n)
    Rd = mandel_rotation(rotations(n, seed + 1))
    Rs = mandel_rotation(rotations(n, seed + 2))
    return rotate_vec(Rd, embed(pool_d[idx] * scale)), rotate_vec(Rs, embed(pool_s[idx]))


def rel_errors(got, ref, sel):
    """(worst tangent error / max|C|, worst stress error / max(|sigma|, 1)) over the selected points."""
    if not np.any(sel):
        return 0.0, 0.0
    eC = np.max(np.abs(got[0][sel] - ref[0][sel])) / np.max(np.abs(ref[0][sel]))
    eS = np.max(np.abs(got[1][sel] - ref[1][sel])) / max(np.max(np.abs(ref[1][sel])), 1.0)
    return float(eC), float(eS)


def rotated_plane_strain(oracle, n, seed, shear=0.0, nthreads=8):
    """The plane-strain tracing inputs embedded and turned by a rotation per point, with what the reference-pinned 2-D oracle says
    about them: its result, the long-double referee's, and the plastic points whose iteration count does not depend on where the
    tolerance sits (the same count at tol = 2e-8, 1e-8 and 5e-9) — the tangent differentiates the iterates, so only there is it
    comparable across arithmetics."""
    from conftest import mc_tracing_inputs

    deps, sn = mc_tracing_inputs(oracle, n, seed=seed, shear=shear)
    ref = oracle.mohr_coulomb(deps, sn, nthreads=nthreads)
    it_hi = oracle.mohr_coulomb(deps, sn, nthreads=nthreads, tangent=False, tol=2e-8)[2]
    it_lo = oracle.mohr_coulomb(deps, sn, nthreads=nthreads, tangent=False, tol=5e-9)[2]
    ld = oracle.mohr_coulomb_long_double(deps, sn, nthreads=nthreads)
    plastic = ~(ref[3] <= 0.0)
    kept = plastic & (it_hi == ref[2]) & (it_lo == ref[2])
    R = mandel_rotation(rotations(len(deps), seed + 100))
    return {"deps": deps, "sn": sn, "ref": ref, "ld": ld, "plastic": plastic, "kept": kept, "R": R,
            "deps6": rotate_vec(R, embed(deps)), "sn6": rotate_vec(R, embed(sn))}


def back_rotated(R, got):
    """A 3-D result in the frame of the plane-strain problem: (R^T C R, R^T sigma)."""
    Rt = np.swapaxes(R, 1, 2)
    return rotate_mat(Rt, got[0]), rotate_vec(Rt, got[1])
