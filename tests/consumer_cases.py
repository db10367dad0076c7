"""Meshes, inputs and bounds shared by tests/test_consumer_reference_cpu.py and tests/test_consumer_reference_gpu.py (not a test module).

The bound of both files is componentwise: |got[k] - ref[k]| <= c * 2^-53 * mag[k] for EVERY dof k, with ref and mag from
oracle/consumer_reference.py (long double). c is not tuned on the kernels: C_REF below is what float64 NumPy itself loses against
long double on these meshes (measured and asserted in test_consumer_reference_cpu.py, per element in its docstrings), and the
kernels get MARGIN = 8 times that for another summation order and fused multiply-adds.
"""
import types

import numpy as np

from tools.synthetic import gauss_tensor_rule, structured_mesh, with_rule

# cells per wave (64 // nq of the degree-2 rules): 21 triangles, 16 quadrilaterals, 16 tetrahedra, 8 hexahedra
# a: one partial wave group; b: full groups plus a ragged tail, interior vertices (non-affine geometry); c: an exact multiple, no tail;
# d: about ten groups, so the eight slices of xcd_group_walk are uneven and some hold two groups
SIZES = {"triangle": {"a": (1, 1), "b": (4, 3), "c": (7, 3), "d": (10, 10)},
         "quadrilateral": {"a": (1, 1), "b": (6, 3), "c": (4, 4), "d": (13, 12)},
         "tetrahedron": {"a": (1, 1, 1), "b": (3, 2, 2), "c": (2, 2, 2), "d": (3, 3, 3)},
         "hexahedron": {"a": (1, 1, 1), "b": (3, 2, 2), "c": (2, 2, 2), "d": (7, 4, 3)}}
# (cell, degree, n, points per direction of the rule or None for quadrature_degree2, size letter)
MUST_SERVE = [(cell, degree, SIZES[cell][s], None, s) for cell in SIZES for degree in (1, 2) for s in "abcd"]
# 9-point rule: 7 cells per wave and one idle lane, 15 cells; 27-point rule: 2 cells per wave and ten idle lanes, 3 and 5 cells
OTHER_RULES = [("quadrilateral", degree, (5, 3), 3, "r") for degree in (1, 2)] + \
              [("hexahedron", degree, n, 3, "r") for degree in (1, 2) for n in ((3, 1, 1), (5, 1, 1))]
ALL_CASES = MUST_SERVE + OTHER_RULES


def case_id(case):
    cell, degree, n, rule, size = case
    return f"{cell}-{'PQ'[cell in ('quadrilateral', 'hexahedron')]}{degree}-{size}{'x'.join(map(str, n))}" + (f"-gauss{rule}" if rule else "")


def element_name(case):
    return f"{case[0]} {'PQ'[case[0] in ('quadrilateral', 'hexahedron')]}{case[1]}" + (f" gauss{case[3]}" if case[3] else "")


# von Mises parameters of the state-based forms (H as oracle/consumer_reference.py::numpy_expand_tangent fixes it: E_t = E / 100)
VM = types.SimpleNamespace(E=70e3, nu=0.3, sigma_0=250.0, H=70e3 * 700.0 / (70e3 - 700.0))

# What float64 NumPy loses against long double, in units of 2^-53 * mag[k], worst dof of every mesh of ALL_CASES; rounded up from the
# figures test_consumer_reference_cpu.py measures, which asserts that they still hold. The large ones belong to the 13 x 12
# quadrilaterals: J is a difference of coordinates of size 1 at a spacing of 1 / 13, which mag does not see and every float64 evaluation,
# the kernels' included, loses alike:
#   apply / force: oracle.operand_oracle.tangent_apply / operand_adjoint;  diag: the float64 twin of ref_tangent_diagonal;
#   apply_vm / diag_vm: the same two fed the float64 tangent-from-state (oracle/consumer_reference.py::numpy_expand_tangent)
C_REF = {"apply": 7.7, "force": 15.0, "diag": 17.2, "apply_vm": 6.4, "diag_vm": 19.4}
MARGIN = 8.0      # another summation order, fused multiply-adds; no other justification


def build_mesh(case):
    cell, degree, n, rule, _ = case
    m = structured_mesh(cell, n, degree, distort=0.2, seed=6)
    return with_rule(m, *gauss_tensor_rule(cell, rule)) if rule else m


def make_inputs(case, mesh, seed=None):
    """Seeded caller-side data of one case: C SPD and different at every point (A A^T + 3 I), v, S, r0 ~ N(0, 1), sigma ~ N(0, 100),
    dp exactly 0.0 on about half the points and |N(0, 1e-3)| on the rest; sizes b and d: the cells of wave group 0 all elastic, those of
    group 1 all plastic (the kernels branch per wave on neither, and must not start to without this noticing). seed: for a case outside
    ALL_CASES (trip_cases.py), whose place in that list is otherwise the seed."""
    G, nn = mesh.gdim, mesh.node_x.shape[0]
    d = 4 if G == 2 else 6
    nc, nq = mesh.num_cells, mesh.nq
    rng = np.random.Generator(np.random.PCG64(20 + ALL_CASES.index(case) if seed is None else seed))
    A = rng.normal(size=(nc, nq, d, d))
    C = A @ A.transpose(0, 1, 3, 2) + 3.0 * np.eye(d)
    sigma = rng.normal(0.0, 100.0, size=(nc, nq, d))
    dp = np.where(rng.random((nc, nq)) < 0.5, 0.0, np.abs(rng.normal(0.0, 1e-3, size=(nc, nq))))
    if case[4] in "bd":
        cpw = 64 // nq
        assert nc > cpw
        dp[:cpw] = 0.0
        dp[cpw:2 * cpw] = np.abs(rng.normal(0.0, 1e-3, size=dp[cpw:2 * cpw].shape)) + 1e-6
    return types.SimpleNamespace(C=np.ascontiguousarray(C), v=rng.normal(size=nn * G), S=rng.normal(size=(nc, nq, d)), sigma=sigma, dp=dp,
                                 r0=rng.normal(size=nn * G), d=d)
