"""Sample points, quadrature rules, meshes and bounds shared by tests/test_hyper3_reference_cpu.py and
tests/test_hyper3_reference_gpu.py (not a test module).

The bound of both files is per entry: |got[k] - ref[k]| <= c * eps * mag[k] for EVERY one of the 9 + 81 outputs of EVERY point, with
ref and mag from oracle/hyper3_reference.py (long double) and eps = 2^-53 (2^-24 for the kernels whose network runs in float32);
entries with mag = 0 must be exact zeros. c is not tuned on the kernels: C_REF below is what the float64 twin of the reference loses
against long double on the sample sets of this file, and the kernels get MARGIN = 8 times that, as in consumer_cases.py.
"""
import concurrent.futures
import functools
import pathlib

import numpy as np

import hyper3_cases as H3
from consumer_cases import MARGIN  # noqa: F401  (the project's figure, shared with the test modules)
from tools.synthetic import gauss_tensor_rule, structured_mesh, with_rule

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
EPS64, EPS32 = 2.0 ** -53, 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- sample sets
def near_identity(n, seed=41):
    """I + 1e-8 N(0, 1): where I1bar - 3, I2bar - 3 and J - 1 cancel"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return H3.EYE + 1e-8 * rng.normal(size=(n, 9))


def rotations(n, seed=43):
    """proper rotations (QR of a normal matrix, the sign of one column fixed): P is analytically 0"""
    rng = np.random.Generator(np.random.PCG64(seed))
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    assert np.allclose(np.linalg.det(Q), 1.0)
    return np.ascontiguousarray(Q.reshape(n, 9))


def near_singular(n, seed=47):
    """large_stretch draws whose smallest singular value is scaled so that det F is log-uniform in [1e-3, 1e-2]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = H3.large_stretch(n, seed=seed).reshape(n, 3, 3)
    U, s, Vt = np.linalg.svd(F)
    target = 10.0 ** rng.uniform(-3.0, -2.0, n)
    s[:, 2] *= target / np.linalg.det(F)
    F = np.einsum("nij,nj,njk->nik", U, s, Vt).reshape(n, 9)
    d = H3.det_rows(F)
    assert d.min() >= 0.99e-3 and d.max() <= 1.01e-2
    return np.ascontiguousarray(F)


def inverted_rows(n, seed=61):
    """small strains; every third row has F_00 lowered by 2.2 and with it det F < 0: NaN in all 90 outputs of the analytic model in
    those rows and in no other, finite in the network operator (J = |det F|)"""
    F = H3.small_strain(n, seed=seed).copy()
    F[1::3, 0] -= 2.2
    d = H3.det_rows(F)
    assert d[1::3].max() < 0.0 and np.delete(d, np.s_[1::3]).min() > 0.5
    return F


def _mixed(n):
    return np.concatenate([H3.small_strain(n // 2, seed=53), H3.large_stretch(n - n // 2, seed=59)])


@functools.lru_cache(maxsize=None)
def sample_sets():
    """name -> F (n, 9), n <= 1000, read-only. The determinant is positive in every set but the last."""
    g = np.load(GOLDEN / "isihara_analytic.npz")
    sets = {"fixed points": H3.fixed_points(),
            "small strain": H3.small_strain(300),
            "large stretch": H3.large_stretch(300),
            "near identity": near_identity(200),
            "rotations": rotations(64),
            "near singular": near_singular(200),
            "scaled by 8": 8.0 * _mixed(200),
            "scaled by 1/8": _mixed(200) / 8.0,
            "plane strain": H3.embed_plane_strain(g["F"][:100]),
            "inverted rows": inverted_rows(130)}
    for name, F in sets.items():
        sets[name] = F = np.ascontiguousarray(F, dtype=np.float64)
        assert F.shape[0] <= 1000 and (name == "inverted rows" or H3.det_rows(F).min() > 0.0), name
        F.setflags(write=False)
    return sets


HARD_SETS = ("near identity", "near singular", "scaled by 8", "scaled by 1/8")
SIZES = (1, 63, 64, 65, 129, None)          # points of a plain call; None: the whole set


@functools.lru_cache(maxsize=None)
def weights():
    return dict(np.load(GOLDEN / "icnn_isihara_weights.npz"))


# What the float64 twin of oracle/hyper3_reference.py (the same code with dtype = np.float64) loses against the long-double reference, in units of
# 2^-53 * mag[k], at the worst entry of the worst point over every sample set above; the two "fp32" figures: what the route with the
# float32 network of oracle.icnn_oracle.network_jets loses against the long-double network, in units of 2^-24 * mag[k]. Rounded up
# from what test_hyper3_reference_cpu.py measures, which asserts that they hold and that none is more than four times the measured.
# Measured (x86-64 long double), and the set that gives the figure:
#   isihara3 P     5.43  scaled by 8          icnn3 fp64 P   12.70  scaled by 8          icnn3 fp32 P   5.01  scaled by 8
#   isihara3 dP    7.76  near identity        icnn3 fp64 dP  22.11  near identity        icnn3 fp32 dP  5.01  scaled by 8
# For comparison, two float64 arrangements that share no line with the twin lose at most: torch autograd on the energy
# (H3.reference, I3.autograd_stress_tangent) 5.84 / 7.49 (analytic model) and 19.92 / 21.22 (network); the jets route of
# icnn3_cases.icnn3_stress_tangent 20.35 / 21.19. The figures belong to float64, not to one ordering.
C_REF = {"isihara3 P": 5.5, "isihara3 dP": 7.8, "icnn3 fp64 P": 12.8, "icnn3 fp64 dP": 22.2, "icnn3 fp32 P": 5.1, "icnn3 fp32 dP": 5.1}


@functools.lru_cache(maxsize=None)
def reference(model, name):
    """(P, dP, magP, magdP) in long double of one sample set, computed once and read-only; model: "isihara3" or "icnn3" (the network in
    long double: what every network kernel is held to, the float32 ones in units of 2^-24)"""
    from oracle.hyper3_reference import icnn3_ref, isihara3_ref

    F = sample_sets()[name]
    out = isihara3_ref(F, H3.DEFAULTS) if model == "isihara3" else icnn3_ref(F, weights())
    for a in out:
        a.setflags(write=False)
    return out


def worst_entry(got, ref, mag, eps, extra=None):
    """(ratio, point, entry): the largest |got - ref| / (eps * mag (+ extra)) over every entry of every point, in long double, and
    where it is. An entry with a zero scale must agree exactly (ratio inf otherwise); a NaN of the reference must be a NaN (inf)."""
    LD = np.longdouble
    n = np.shape(ref)[0]
    got, ref = np.asarray(got, dtype=LD).reshape(n, -1), np.asarray(ref, dtype=LD).reshape(n, -1)
    scale = LD(eps) * np.asarray(mag, dtype=LD).reshape(n, -1) + (0 if extra is None else np.asarray(extra, dtype=LD).reshape(n, -1))
    if got.size == 0:
        return 0.0, -1, -1
    nan = np.isnan(ref)
    err = np.where(nan, 0, np.abs(got - np.where(nan, 0, ref)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0, np.inf))
    ratio = np.where(nan, np.where(np.isnan(got), 0, np.inf), ratio)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    p, k = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[p, k]), int(p), int(k)


# ------------------------------------------------------------------------------------------------- rules and meshes of the fused form
# Interior points with positive weights (the operator does not integrate; the weights sum to the volume 1 / 6 all the same).
# 7 points: the barycentre and the six permutations of the barycentric coordinates (0.1, 0.1, 0.4, 0.4);
# 11 points: those and the four permutations of (0.1, 0.1, 0.1, 0.7).
_A, _B, _C = 0.1, 0.4, 0.7
TET7 = np.array([[0.25, 0.25, 0.25], [_A, _A, _B], [_A, _B, _A], [_B, _A, _A], [_A, _B, _B], [_B, _A, _B], [_B, _B, _A]])
TET11 = np.concatenate([TET7, [[_A, _A, _A], [_C, _A, _A], [_A, _C, _A], [_A, _A, _C]]])


def tet_rule(nq):
    pts = {7: TET7, 11: TET11}[nq]
    return np.ascontiguousarray(pts), np.full(nq, 1.0 / (6.0 * nq))


def hex_tensor_rule(npx, npy, npz):
    """Gauss-Legendre with npx x npy x npz points on the unit cube, x fastest (gauss_tensor_rule has one count for all directions)"""
    rules = [np.polynomial.legendre.leggauss(k) for k in (npx, npy, npz)]
    (tx, wx), (ty, wy), (tz, wz) = [(0.5 * (t + 1.0), 0.5 * w) for t, w in rules]
    pts = np.array([[x, y, z] for z in tz for y in ty for x in tx])
    wts = np.array([a * b * c for c in wz for b in wy for a in wx])
    return pts, wts


# name -> (cell, n, degree, rule): rule None (the degree-2 rule), an int (gauss_tensor_rule), ("tet", nq) or ("hex", nx, ny, nz)
FUSED_MESHES = {
    # the seven of test_hyper3_gpu.MESHES
    "Q2 hexahedra (2,1,2), 8 points": ("hexahedron", (2, 1, 2), 2, None),
    "Q2 hexahedra (3,3,2), 8 points": ("hexahedron", (3, 3, 2), 2, None),
    "Q2 hexahedra (2,1,2), 27 points": ("hexahedron", (2, 1, 2), 2, 3),
    "Q2 hexahedra (3,3,2), 27 points": ("hexahedron", (3, 3, 2), 2, 3),
    "Q1 hexahedra (3,2,3)": ("hexahedron", (3, 2, 3), 1, None),
    "P2 tetrahedra (2,2,1)": ("tetrahedron", (2, 2, 1), 2, None),
    "P1 tetrahedra (3,2,2)": ("tetrahedron", (3, 2, 2), 1, None),
    # an odd number of points per wave group: 55 (11 points, 5 cells), 63 (7 points, 9 cells; 9 points, 7 cells)
    "P2 tetrahedra (2,2,1), 11 points": ("tetrahedron", (2, 2, 1), 2, ("tet", 11)),
    "P2 tetrahedra (2,2,1), 7 points": ("tetrahedron", (2, 2, 1), 2, ("tet", 7)),
    "P1 tetrahedra (3,2,2), 11 points": ("tetrahedron", (3, 2, 2), 1, ("tet", 11)),
    "P1 tetrahedra (3,2,2), 7 points": ("tetrahedron", (3, 2, 2), 1, ("tet", 7)),
    "Q1 hexahedra (3,2,3), 3x3x1 points": ("hexahedron", (3, 2, 3), 1, ("hex", 3, 3, 1)),
    # another pass length of the tangent stores (pass_points below): 13, odd, so that the passes of one group alternate in parity
    "Q2 hexahedra (2,1,2), 7x2x2 points": ("hexahedron", (2, 1, 2), 2, ("hex", 7, 2, 2)),
}
ODD_GROUP_MESHES = [name for name in FUSED_MESHES if name.endswith((", 11 points", ", 7 points", "3x3x1 points"))]
assert len(ODD_GROUP_MESHES) == 5
# for the host call in chunks: the host pipeline cuts on multiples of 64 cells, so three chunks need more than 128 cells
CHUNK_MESHES = {"P1 tetrahedra (4,3,2), 7 points": ("tetrahedron", (4, 3, 2), 1, ("tet", 7)),
                "P1 tetrahedra (4,3,2), 11 points": ("tetrahedron", (4, 3, 2), 1, ("tet", 11))}
CHUNK_CELLS = 64


def _trip_mesh(name):
    """a mesh of trip_cases.CASES (many wave groups: tests/test_trips_gpu.py), taken by name like the ones above"""
    return name not in FUSED_MESHES and name not in CHUNK_MESHES


def fused_mesh(name):
    if _trip_mesh(name):
        import trip_cases

        return trip_cases.mesh(name)
    cell, n, degree, rule = FUSED_MESHES[name] if name in FUSED_MESHES else CHUNK_MESHES[name]
    m = structured_mesh(cell, n, degree, distort=0.2, seed=4)
    if rule is None:
        return m
    if isinstance(rule, int):
        return with_rule(m, *gauss_tensor_rule(cell, rule))
    return with_rule(m, *(tet_rule(rule[1]) if rule[0] == "tet" else hex_tensor_rule(*rule[1:])))


def pass_points(m):
    """pp of the fused Isihara kernel's tangent passes, as isi3_field_launch (csrc/hyper3.hip) computes it from the mesh's LDS tables:
    table_doubles as dxo_mesh_create lays them out (phi, dphi, dpsi rows padded to an odd length), a quarter of the remaining 64 KiB
    per wave, 81 doubles per point and 2 for the parity slot"""
    odd = lambda k: k | 1                                                    # noqa: E731
    nd, ng, G = m.dofmap.shape[1], m.geom_dofmap.shape[1], m.gdim
    table = (m.nq * (odd(nd) + odd(nd * G) + odd(ng * G)) + 1) & ~1
    room = ((8192 - table) // 4) & ~1
    return min(16, (room - 2) // 81), table


def group_starts(m):
    """first point of every wave group of the fused kernels (cells_per_wave = 64 // nq cells each) and the points of each"""
    cpw = 64 // m.nq
    first = np.arange(0, m.num_cells, cpw)
    return first * m.nq, np.minimum(cpw, m.num_cells - first) * m.nq


@functools.lru_cache(maxsize=None)
def fused_reference(model, name):
    """What a fused call on the mesh `name` is held to, computed once and read-only: (u, P, dP, magP, magdP, extraP, extradP).
    F comes from the long-double operand reference at the field u (test_hyper3_gpu._field, amplitude 0.15), ref = model(F_LD), and
    extra is the allowance for the float64 rounding of F that tests/test_operand_reference_gpu.py grants the operand kernels,
        extra[k] = sum_j |d ref[k] / d F_j| * MARGIN * C_REF["F"] * 2^-53 * magF_j,
    with dP/dF the reference's own dP and d(dP)/dF a central difference of the long-double reference at the step 2^-20 (its
    truncation, 2^-40 of the fourth derivative, is far below what an allowance needs). On a mesh of trip_cases.CASES the C_REF["F"] is
    trip_cases.C_REF_TRIP["F"], what the operand test grants on that mesh."""
    import operand_cases as OC
    from oracle.hyper3_reference import LD, icnn3_ref, isihara3_ref
    from oracle.operand_reference import ref_operand
    from test_hyper3_gpu import _field

    m = fused_mesh(name)
    u = _field(m, 0.15, 9)
    if _trip_mesh(name):
        import trip_cases

        u = trip_cases.hyper3_field_u(name)
    F, magF = (a.reshape(-1, 9) for a in ref_operand(m, "F", 3, u))
    f = (lambda X: isihara3_ref(X, H3.DEFAULTS)) if model == "isihara3" else (lambda X: icnn3_ref(X, weights()))
    P, dP, mP, mdP = f(F)
    assert np.isfinite(np.asarray(dP, dtype=np.float64)).all()
    c_ref_F = OC.C_REF["F"]
    if _trip_mesh(name):
        c_ref_F = trip_cases.C_REF_TRIP["F"][0]
    cF = LD(OC.MARGIN * c_ref_F) * LD(2.0) ** -53
    extraP = np.einsum("nkj,nj->nk", np.abs(dP), magF) * cF
    h, n = LD(2.0) ** -20, F.shape[0]
    extradP = np.zeros((n, 81), dtype=LD)

    def leg(j):          # |d(dP) / dF_j| magF_j
        Fp, Fm = F.copy(), F.copy()
        Fp[:, j] += h
        Fm[:, j] -= h
        return np.abs((f(Fp)[1] - f(Fm)[1]) / (2 * h)).reshape(n, 81) * magF[:, j:j + 1]

    # the nine legs are independent and NumPy releases the interpreter lock inside its loops: on the trip meshes (5000 points) the
    # threads bring the reference from 10 s to a few; the sum is taken in the order j = 0 .. 8 as before
    with concurrent.futures.ThreadPoolExecutor(max_workers=9) as pool:
        for term in pool.map(leg, range(9)):
            extradP += term
    out = (u, P, dP, mP, mdP, extraP, (extradP * cF).reshape(n, 9, 9))
    for a in out:
        a.setflags(write=False)
    return out
