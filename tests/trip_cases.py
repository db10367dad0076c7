"""Meshes, the replay of the group walk, inputs, references and bounds shared by tests/test_trips_cpu.py and tests/test_trips_gpu.py (not
a test module).

A TRIP is one pass of a wave through the body of `for (grp = walk.first; grp < walk.end; grp += walk.stride)` (xcd_group_walk,
csrc/operand_core.h): the persistent element kernels give a wave one wave group of cells_per_wave = 64 // nq cells per trip (64 cells
in the lane = cell strain kernel of operand_cell.h). wave_group_grid (csrc/form_host.h) launches a workgroup of four waves per four
groups, at most blocks_per_cu per compute unit, so on an MI355X a wave takes a second trip only past 4 * 8 * 256 = 8192 groups. The
option "wave_group_blocks" caps the grid instead: at 8 every one of the 8 XCD slices is walked by ONE workgroup, and a mesh of about
75 groups sends every wave round the loop two or three times — the steady state of the two-deep register pipelines
(pipe_load_values / pipe_load_indices inside the loop), the op_fence() that lets the next trip overwrite the wave's LDS region, and
group_cells() = 0 for a look-ahead past the end of the slice while earlier groups are still in flight.

walk() replays the grid rounding and the walk; it is used to assert preconditions (check_trips) and to split reported ratios into
first-trip and later-trip cells (later_trip_mask), never as a reference for results.

Bounds. Where a long-double reference exists the bound is the project's componentwise one, |got[k] - ref[k]| <= MARGIN * C * 2^-53 *
mag[k] (+ extra[k]); C is what the float64 twin of the same reference loses against long double ON THESE MESHES (C_REF_TRIP below,
measured and asserted in test_trips_cpu.py: the loss grows with 1 / h through the Jacobian's cancelling coordinate differences, so the
figures of consumer_cases / operand_cases, measured on coarser meshes, need not hold here), MARGIN = 8 from consumer_cases. Where only
a float64 oracle exists the bound is the one the kernel's small-mesh test states against that oracle (TOL_* below).
"""
import functools
import types

import numpy as np

import consumer_cases as CC
import hyper3_cases as H3
import operand_cases as OC
from consumer_cases import MARGIN, VM  # noqa: F401  (shared with the test modules)
from tools.synthetic import gauss_tensor_rule, structured_mesh, with_rule

XCDS = 8
OPTIONS = (8, 16, 0)                  # wave_group_blocks of every GPU test: three trips, two trips, the default grid (one trip)
MI355X_COMPUTE_UNITS = 256

# name -> (cell, degree, n, rule, "t"): the tuple of consumer_cases (rule: None = the degree-2 rule, 3 = 3 Gauss points per direction,
# "centroid" = the one-point rule with weight = the reference cell's volume)
CASES = {
    "P1 triangles (28,28)": ("triangle", 1, (28, 28), None, "t"),
    "P2 triangles (28,28)": ("triangle", 2, (28, 28), None, "t"),
    "Q2 quadrilaterals (35,33)": ("quadrilateral", 2, (35, 33), None, "t"),
    "Q2 quadrilaterals (27,25), gauss 3": ("quadrilateral", 2, (27, 25), 3, "t"),
    "P1 tetrahedra (7,6,5)": ("tetrahedron", 1, (7, 6, 5), None, "t"),
    "P2 tetrahedra (7,6,5)": ("tetrahedron", 2, (7, 6, 5), None, "t"),
    "Q1 hexahedra (11,9,6)": ("hexahedron", 1, (11, 9, 6), None, "t"),
    "Q2 hexahedra (11,9,6)": ("hexahedron", 2, (11, 9, 6), None, "t"),
    "Q1 hexahedra (7,7,3), gauss 3": ("hexahedron", 1, (7, 7, 3), 3, "t"),
    "Q2 hexahedra (7,7,3), gauss 3": ("hexahedron", 2, (7, 7, 3), 3, "t"),
    # cells_per_wave = 64 with 4 (3) vertices each: 256 (192) vertex slots > OP_XI * 64, so operand_can_pipe is false and the kernels
    # that ask it take their gather-in-the-loop form. dxo_mesh_create serves nq = 1, and so do the operand, heat and von Mises field
    # kernels; the array forms of adjoint.hip and bilinear.h refuse the tetrahedra for the LDS budget (64 cells' dofs and vertices per
    # wave). No other rule on P1 tetrahedra has cells_per_wave * ngeom > 128, so the triangles stand beside them: 64 cells need 896
    # doubles per wave there instead of 1664. What still refuses is asserted as a refusal (test_trips_gpu.LDS_REFUSED)
    "P1 tetrahedra (10,10,9), 1 point": ("tetrahedron", 1, (10, 10, 9), "centroid", "t"),
    # for the lane = cell strain kernel, whose group is 64 cells
    "P2 triangles (50,47)": ("triangle", 2, (50, 47), None, "t"),
    "Q2 quadrilaterals (69,68)": ("quadrilateral", 2, (69, 68), None, "t"),
    # the second mesh without a register pipeline (see above)
    "P1 triangles (60,45), 1 point": ("triangle", 1, (60, 45), "centroid", "t"),
}
NO_PIPE = ("P1 tetrahedra (10,10,9), 1 point", "P1 triangles (60,45), 1 point")
LANE_CELL = ("P2 triangles (50,47)", "Q2 quadrilaterals (69,68)")          # 4700 cells / 74 groups, 4692 cells / 74 groups
WAVE_GROUP = [name for name in CASES if name not in LANE_CELL]              # the meshes of the wave-group kernels
PIPED = [name for name in WAVE_GROUP if name not in NO_PIPE]
HYPER3 = ["P2 tetrahedra (7,6,5)", "Q2 hexahedra (11,9,6)", "Q2 hexahedra (7,7,3), gauss 3", "Q1 hexahedra (11,9,6)",
          "P1 tetrahedra (7,6,5)", "Q1 hexahedra (7,7,3), gauss 3"]
# (the array-free hyperelastic forms have an unpiped branch too, but no 3-D mesh reaches it: the one-point tetrahedra need 2496 doubles
# per wave in the residual and the action and 2048 in the diagonal, 79.9 and 65.8 KB with the tables, and are refused)
HYPER3_FIELD = ["P2 tetrahedra (7,6,5)", "Q2 hexahedra (11,9,6)", "Q2 hexahedra (7,7,3), gauss 3", "P1 tetrahedra (7,6,5)"]
# the table of the issue: (cells, cells per wave, groups, cells of the ragged last group)
EXPECTED = {"P1 triangles (28,28)": (1568, 21, 75, 14), "P2 triangles (28,28)": (1568, 21, 75, 14),
            "Q2 quadrilaterals (35,33)": (1155, 16, 73, 3), "Q2 quadrilaterals (27,25), gauss 3": (675, 7, 97, 3),
            "P1 tetrahedra (7,6,5)": (1260, 16, 79, 12), "P2 tetrahedra (7,6,5)": (1260, 16, 79, 12),
            "Q1 hexahedra (11,9,6)": (594, 8, 75, 2), "Q2 hexahedra (11,9,6)": (594, 8, 75, 2),
            "Q1 hexahedra (7,7,3), gauss 3": (147, 2, 74, 1), "Q2 hexahedra (7,7,3), gauss 3": (147, 2, 74, 1),
            "P1 tetrahedra (10,10,9), 1 point": (5400, 64, 85, 24), "P1 triangles (60,45), 1 point": (5400, 64, 85, 24), "P2 triangles (50,47)": (4700, 64, 74, 28),
            "Q2 quadrilaterals (69,68)": (4692, 64, 74, 20)}

# Float64 oracles only: the figure the kernel's small-mesh test states, of max |ref|
TOL_BILINEAR = 1e-12          # tests/test_bilinear_gpu.py
TOL_HYPER3_MF = 1e-12         # tests/test_hyper3_mf_gpu.py
TOL_VM_FIELD = 1e-12          # tests/test_operand_eval.py::test_fused_operand_plus_von_mises
TOL_HEAT_FIELD = 1e-13        # tests/test_operand_eval.py::test_value_and_gradient_in_one_pass_and_fused_heat
TOL_ISIHARA_FIELD = 1e-12     # tests/test_icnn.py::test_isihara_hip_against_golden_and_oracle (oracle.icnn_oracle.isihara_stress_tangent)

# What the float64 twin of each reference loses against long double, in units of 2^-53 * mag[k], at the worst entry over the trip meshes
# that serve the entry: key -> (figure, the mesh that gives it). Rounded up from what test_trips_cpu.py measures, which asserts that
# they hold and that none is more than four times the measured figure (the rule of hyper3_reference_cases.py). Twins: operand kinds —
# oracle.operand_oracle.eval_operand, field "rough", bs = 1 and gdim; apply / force — oracle.operand_oracle.tangent_apply /
# operand_adjoint; diag — the float64 twin of ref_tangent_diagonal; apply_vm / diag_vm — the same fed numpy_expand_tangent; isihara3 —
# the float64 twin of oracle.hyper3_reference.isihara3_ref at the float64 rounding of the long-double F of HYPER3_FIELD.
# Measured (x86-64 long double):
#   value        5.10  Q2 hexahedra (7,7,3), gauss 3            apply      20.36  Q2 quadrilaterals (35,33)
#   grad       258.52  Q2 quadrilaterals (27,25), gauss 3       force      40.11  the same
#   value_grad 258.52  the same                                 diag       50.91  the same
#   eps        220.19  the same                                 apply_vm   31.47  the same
#   F          138.30  the same                                 diag_vm    61.17  the same
#   C           88.82  the same                                 isihara3 P  2.45  P2 tetrahedra (7,6,5)
#   I1          24.47  the same                                 isihara3 dP 6.01  the same
#   detF        19.79  the same
# Against operand_cases.C_REF (grad 44.6 at a spacing of 1 / 13) and consumer_cases.C_REF (diag 17.2): the quadrilaterals at a spacing
# of 1 / 27 and 1 / 35 lose three to six times as much in J, as consumer_cases.py predicts; the hexahedra reach 52 in the gradient (27-point
# rule), the simplices stay below 20 (test_trips_cpu.py prints the figures of every mesh).
_QG3, _Q = "Q2 quadrilaterals (27,25), gauss 3", "Q2 quadrilaterals (35,33)"
C_REF_TRIP = {"value": (5.2, "Q2 hexahedra (7,7,3), gauss 3"), "grad": (258.6, _QG3), "value_grad": (258.6, _QG3), "eps": (220.2, _QG3),
              "F": (138.4, _QG3), "C": (88.9, _QG3), "I1": (24.5, _QG3), "detF": (19.8, _QG3),
              "apply": (20.4, _Q), "force": (40.2, _Q), "diag": (51.0, _Q), "apply_vm": (31.5, _Q), "diag_vm": (61.2, _Q),
              "isihara3 P": (2.5, "P2 tetrahedra (7,6,5)"), "isihara3 dP": (6.1, "P2 tetrahedra (7,6,5)")}


def case_cpw(name):
    """cells of a wave group of the kernels that serve the mesh `name`"""
    return 64 if name in LANE_CELL else 64 // mesh(name).nq


@functools.lru_cache(maxsize=None)
def mesh(name):
    cell, degree, n, rule, _ = CASES[name]
    m = structured_mesh(cell, n, degree, distort=0.2, seed=6)
    if rule == "centroid":          # one point at the centroid, weight = the reference cell's volume
        G = m.gdim
        return with_rule(m, np.full((1, G), 1.0 / (G + 1)), np.array([1.0 / 2.0 if G == 2 else 1.0 / 6.0]))
    return with_rule(m, *gauss_tensor_rule(cell, rule)) if rule else m


def seed_of(name):
    return 5000 + 100 * list(CASES).index(name)


# ------------------------------------------------------------------------------------------------ the walk
def grid_blocks(n_groups, blocks, blocks_per_cu=8, compute_units=MI355X_COMPUTE_UNITS):
    """wave_group_grid: ceil(n_groups / 4) workgroups, at most `blocks` (0: blocks_per_cu per compute unit), rounded up to whole rounds
    over the 8 XCDs"""
    cap = blocks if blocks > 0 else blocks_per_cu * compute_units
    return (min(-(-n_groups // 4), cap) + XCDS - 1) // XCDS * XCDS


def walk(n_groups, blocks, waves=4):
    """{(block, wave): [groups in the order the wave visits them]} of a launch over n_groups wave groups with option
    wave_group_blocks = blocks: xcd_group_walk on the grid of wave_group_grid. Workgroup b belongs to XCD b % 8, which owns the
    contiguous slice [n_groups * xcd // 8, n_groups * (xcd + 1) // 8); its workgroups stride through it together."""
    grid = grid_blocks(n_groups, blocks)
    per_xcd = grid // XCDS
    out = {}
    for b in range(grid):
        xcd, local = b % XCDS, b // XCDS
        begin, end = n_groups * xcd // XCDS, n_groups * (xcd + 1) // XCDS
        for w in range(waves):
            out[(b, w)] = list(range(begin + local * waves + w, end, per_xcd * waves))
    return out


def trip_of_group(n_groups, blocks):
    """trip[g] = 0 for the first group of its wave, 1 for the second, ...; prev[g] = the group the same wave visited one trip earlier
    (-1 on trip 0)"""
    trip, prev = np.full(n_groups, -1), np.full(n_groups, -1)
    for groups in walk(n_groups, blocks).values():
        for t, g in enumerate(groups):
            assert trip[g] == -1
            trip[g], prev[g] = t, groups[t - 1] if t else -1
    assert (trip >= 0).all()
    return trip, prev


def later_trip_mask(m, blocks, cpw=None):
    """(num_cells,) bool: the cells whose group is not the first of its wave at wave_group_blocks = blocks"""
    cpw = 64 // m.nq if cpw is None else cpw
    trip, _ = trip_of_group(-(-m.num_cells // cpw), blocks)
    return trip[np.arange(m.num_cells) // cpw] > 0


def stale_cells(m, blocks, cpw=None):
    """(num_cells,) the cell whose data a stale pipeline slot would deliver in place of each cell's: the cell at the same place of the
    group the wave visited one trip earlier (a full group: the ragged last one finds every place filled); first-trip cells themselves"""
    cpw = 64 // m.nq if cpw is None else cpw
    cells = np.arange(m.num_cells)
    g = cells // cpw
    _, prev = trip_of_group(-(-m.num_cells // cpw), blocks)
    return np.where(prev[g] >= 0, prev[g] * cpw + cells % cpw, cells)


def check_trips():
    """-> report lines; asserts what the module docstring promises of every mesh"""
    lines = []
    for name in CASES:
        m, cpw = mesh(name), case_cpw(name)
        n_groups = -(-m.num_cells // cpw)
        assert (m.num_cells, cpw, n_groups, m.num_cells - (n_groups - 1) * cpw) == EXPECTED[name], name
        w8 = walk(n_groups, 8)
        assert len(w8) == 8 * 4
        assert sorted(g for groups in w8.values() for g in groups) == list(range(n_groups)), name          # each group exactly once
        trips = {k: len(v) for k, v in w8.items()}
        assert max(trips.values()) >= 3, name
        assert any(len({trips[(b, w)] for w in range(4)}) > 1 for b in range(8)), name     # a look-ahead past the end beside one inside
        assert n_groups % 8 != 0 and m.num_cells % cpw != 0, name                           # uneven slices, a ragged last group
        w16 = walk(n_groups, 16)
        assert len(w16) == 16 * 4 and sorted(g for groups in w16.values() for g in groups) == list(range(n_groups)), name
        assert max(len(v) for v in w16.values()) == 2, name
        w0 = walk(n_groups, 0)
        assert max(len(v) for v in w0.values()) == 1, name                                  # the default grid: one trip, as before
        later = later_trip_mask(m, 8, cpw)
        lines.append(f"{name:36s} {m.num_cells:5d} cells, cpw {cpw:2d}, {n_groups:3d} groups (last {m.num_cells % cpw:2d} cells): trips per wave "
                     f"{min(trips.values())}-{max(trips.values())} at 8, {int(later.sum()):5d} later-trip cells")
    return lines


# ------------------------------------------------------------------------------------------------ operand family
OPERAND_KINDS = ("value", "grad", "eps", "F", "value_grad", "C", "I1", "detF")


def operand_entries(name):
    G = mesh(name).gdim
    return [(kind, bs) for bs in (1, G) for kind in OPERAND_KINDS if bs == G or kind in OC.COMPONENT_KINDS]


@functools.lru_cache(maxsize=None)
def operand_field(name, bs):
    u = OC.fields(CASES[name], mesh(name), bs, seed=seed_of(name))["rough"]
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def operand_reference(name, kind, bs):
    """(ref, mag) in long double over all cells, computed once and read-only"""
    from oracle.operand_reference import ref_operand

    out = ref_operand(mesh(name), kind, bs, operand_field(name, bs))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ consumer family
CONSUMER_ENTRIES = ("apply", "diag", "apply_vm", "diag_vm", "force")


@functools.lru_cache(maxsize=None)
def consumer_inputs(name):
    return CC.make_inputs(CASES[name], mesh(name), seed=seed_of(name) + 7)


def consumer_reference_of(m, x, entry):
    from oracle.consumer_reference import ref_adjoint_eps, ref_tangent_apply, ref_tangent_diagonal, vm_tangent_from_state

    if entry == "apply":
        return ref_tangent_apply(m, x.C, x.v)
    if entry == "diag":
        return ref_tangent_diagonal(m, x.C)
    if entry == "force":
        return ref_adjoint_eps(m, x.S)
    Cvm, Cvm_mag = vm_tangent_from_state(VM, x.sigma, x.dp)
    return ref_tangent_apply(m, Cvm, x.v, C_mag=Cvm_mag) if entry == "apply_vm" else ref_tangent_diagonal(m, Cvm, C_mag=Cvm_mag)


@functools.lru_cache(maxsize=None)
def consumer_reference(name, entry):
    out = consumer_reference_of(mesh(name), consumer_inputs(name), entry)
    for a in out:
        a.setflags(write=False)
    return out


def stale_consumer_inputs(name, blocks):
    """the inputs with the point data (C, S, sigma, dp) of every later-trip cell replaced by its stale cell's"""
    x, src = consumer_inputs(name), stale_cells(mesh(name), blocks)
    return types.SimpleNamespace(C=x.C[src], S=x.S[src], sigma=x.sigma[src], dp=x.dp[src], v=x.v, r0=x.r0, d=x.d)


# ------------------------------------------------------------------------------------------------ hyperelastic field family
def hyper3_c(key):
    return MARGIN * C_REF_TRIP["isihara3 " + key][0]


# ------------------------------------------------------------------------------------------------ float64-oracle families
BILINEAR_PAIRS = (("grad", "grad", True), ("grad", "grad", False), ("eps", "eps", True), ("value", "value", False))


def _vsize(kind, G, bs):
    return {"value": bs, "grad": bs * G, "eps": 4 if G == 2 else 6}[kind]


@functools.lru_cache(maxsize=None)
def bilinear_case(name, pair):
    """(bs, Cb, v, K v) of one pair on the mesh `name`: oracle.form_oracle.bilinear_ref (float64), read-only"""
    from oracle.form_oracle import bilinear_ref

    test, trial, vector = BILINEAR_PAIRS[pair]
    m = mesh(name)
    bs = m.gdim if vector else 1
    rng = np.random.Generator(np.random.PCG64(seed_of(name) + 11 + pair))
    Cb = rng.normal(size=(m.num_cells * m.nq, _vsize(test, m.gdim, bs), _vsize(trial, m.gdim, bs)))
    v = rng.normal(size=m.node_x.shape[0] * bs)
    out = (bs, Cb, v, bilinear_ref(m, test, trial, bs, Cb, v))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bilinear_diagonal(name, pair):
    """diag K of the same pair and block: oracle.form_oracle.bilinear_diag_ref, the action probed one node colour at a time (27 colours
    times bs probes on Q2 hexahedra, 3.5 s: the GPU test forms the pairs of a mesh side by side in threads)"""
    from oracle.form_oracle import bilinear_diag_ref

    test, trial, _ = BILINEAR_PAIRS[pair]
    bs, Cb, _, _ = bilinear_case(name, pair)
    out = bilinear_diag_ref(mesh(name), test, trial, bs, Cb)
    out.setflags(write=False)
    return out


def in_threads(f, args):
    """[f(a) for a in args], side by side: NumPy releases the interpreter lock inside its loops"""
    import concurrent.futures

    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, len(args))) as pool:
        return list(pool.map(f, args))


def hyper3_mf_of(m, F, with_diag=True):
    """residual, action and (with_diag) diagonal of the analytic model from the per-point F (n, 9), as tests/test_hyper3_mf_gpu.case
    forms them"""
    from oracle.form_oracle import bilinear_diag_ref, bilinear_ref, tables
    from oracle.operand_oracle import DEFGRAD, operand_adjoint

    nn, nc, nq = m.node_x.shape[0], m.num_cells, m.nq
    v = np.random.Generator(np.random.PCG64(23)).normal(size=nn * 3)
    P, dP = H3.reference(np.array(F))
    R = operand_adjoint(DEFGRAD, 3, P.reshape(nc, nq, 9), m.weights, *tables(m), nn)
    out = dict(v=v, R=np.asarray(R).reshape(-1), Kv=bilinear_ref(m, "grad", "grad", 3, dP, v))
    if with_diag:
        out["diag"] = bilinear_diag_ref(m, "grad", "grad", 3, dP)
    return out


# The hyperelastic entries run at test_hyper3_gpu._field(m, amplitude, 9) with the amplitude 0.15 of their small tests, where det F > 0.2
# on five of the six 3-D meshes (asserted). On the P2 tetrahedra the field's nodal noise, 0.05 * amplitude at a node spacing of 1 / 14,
# inverts a cell at 0.15 (det F = -0.23 at one point, 0.21 at its smallest with 0.1): there the amplitude is 0.075, det F >= 0.42
HYPER3_AMPLITUDE = {"P2 tetrahedra (7,6,5)": 0.075}


@functools.lru_cache(maxsize=None)
def hyper3_field_u(name):
    from test_hyper3_gpu import _field

    u = _field(mesh(name), HYPER3_AMPLITUDE.get(name, 0.15), 9)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def hyper3_F64(name):
    from oracle.form_oracle import tables
    from oracle.operand_oracle import DEFGRAD, eval_operand

    m = mesh(name)
    F = eval_operand(DEFGRAD, 3, hyper3_field_u(name), *tables(m)).reshape(m.num_cells, m.nq, 9)
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def hyper3_mf_case(name, with_diag=True):
    m, F = mesh(name), hyper3_F64(name)
    out = hyper3_mf_of(m, F.reshape(-1, 9), with_diag)
    out.update(u=hyper3_field_u(name), det_min=float(H3.det_rows(F.reshape(-1, 9)).min()))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- the fused von Mises, heat and 2-D Isihara field entries: the inputs of their small tests scaled to the trip mesh
E_VM = 70e3


@functools.lru_cache(maxsize=None)
def vm_field_case(name):
    """u scaled so that the strain has standard deviation 1.5e-3, (sigma_n, p) as tests/test_operand_eval._vm_state, and the float64
    strain of the operand oracle (the von Mises oracle is applied to it by the caller, which has the `oracle` fixture)"""
    from oracle.form_oracle import tables
    from oracle.operand_oracle import EPS_MANDEL, eval_operand

    m = mesh(name)
    d, npts = 4 if m.gdim == 2 else 6, m.num_cells * m.nq
    rng = np.random.Generator(np.random.PCG64(seed_of(name) + 31))
    u = rng.normal(size=m.node_x.shape[0] * m.gdim)
    u *= 1.5e-3 / eval_operand(EPS_MANDEL, m.gdim, u, *tables(m)).std()
    rng = np.random.Generator(np.random.PCG64(seed_of(name) + 32))
    sigma_n, p = rng.normal(0.0, 50.0, (npts, d)), np.abs(rng.normal(0.0, 1e-3, npts))
    eps = eval_operand(EPS_MANDEL, m.gdim, u, *tables(m)).reshape(m.num_cells, m.nq, d)
    out = types.SimpleNamespace(u=u, sigma_n=sigma_n, p=p, eps=eps, d=d)
    for a in (u, sigma_n, p, eps):
        a.setflags(write=False)
    return out


def heat_of(vg, G):
    """(q, dq/dT, dq/dsigma) of the heat kernels with A = B = 1 from value_grad rows (n, 1 + G): the three formulas of
    demo_nonlinear_heat_equation_part2.py as tests/test_operand_eval.py writes them in NumPy"""
    k = 1.0 / (1.0 + vg[:, 0])
    sg = vg[:, 1:]
    return -k[:, None] * sg, (k * k)[:, None] * sg, np.ascontiguousarray(np.broadcast_to(-k[:, None, None] * np.eye(G)[None], (len(k), G, G)))


@functools.lru_cache(maxsize=None)
def heat_field_case(name):
    from oracle.form_oracle import tables
    from oracle.operand_oracle import VALUE_GRAD, eval_operand

    m = mesh(name)
    G, x = m.gdim, m.node_x
    rng = np.random.Generator(np.random.PCG64(seed_of(name) + 41))
    Tn = 1.0 + x[:, 0] ** 2 + x[:, 1] + (0.3 * x[:, 2] * x[:, 0] if G == 3 else 0.0) + 0.02 * rng.random(x.shape[0])
    vg = eval_operand(VALUE_GRAD, 1, Tn, *tables(m)).reshape(m.num_cells, m.nq, 1 + G)
    for a in (Tn, vg):
        a.setflags(write=False)
    return types.SimpleNamespace(T=Tn, vg=vg)


ISI2 = (0.5, 1.0, 1.0, 1.5)          # IsiharaParams of tests/test_bilinear_gpu.py


@functools.lru_cache(maxsize=None)
def isihara_field_case(name):
    """2-D: u with |grad u| of a few per cent, and the float64 F of the operand oracle"""
    from oracle.form_oracle import tables
    from oracle.operand_oracle import DEFGRAD, eval_operand

    m = mesh(name)
    assert m.gdim == 2
    x = m.node_x
    rng = np.random.Generator(np.random.PCG64(seed_of(name) + 51))
    h = 1.0 / (max(CASES[name][2]) * CASES[name][1])
    u = 0.1 * np.stack([np.sin(2.0 * x[:, 1]) * x[:, 0], np.cos(1.5 * x[:, 0]) * x[:, 1]], axis=1) + 0.05 * h * rng.normal(size=x.shape)
    u = np.ascontiguousarray(u.reshape(-1))
    F = eval_operand(DEFGRAD, 2, u, *tables(m)).reshape(m.num_cells, m.nq, 4)
    for a in (u, F):
        a.setflags(write=False)
    return types.SimpleNamespace(u=u, F=F)
