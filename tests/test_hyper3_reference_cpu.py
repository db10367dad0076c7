"""The 3-D Isihara operator without a GPU: the autograd reference of tests/hyper3_cases.py pinned to the reference's own data through
the plane-strain embedding F = [[F_2, 0], [0, 1]] (tests/golden/isihara_analytic.npz), its invariances, and the C entry points'
behaviour where no device is needed.

A dxo_ctx exists only on a device (dxo_ctx_create answers DXO_E_NODEVICE otherwise), so what can be asked here of the argument checks
is that every bad call answers what its 2-D twin answers on the NULL context both are given; the same list against a real context,
where each check is reached, is tests/test_hyper3_gpu.py::test_bad_arguments_answer_as_the_2d_twins.

The second half of the file is about oracle/hyper3_reference.py, the long-double closed form that tests/test_hyper3_reference_gpu.py
holds the 3-D kernels to entry by entry, and about the constants of tests/hyper3_reference_cases.py."""
import ctypes as C
import types

import numpy as np

import hyper3_cases as H3
from dolfinx_external_operator_amd import IsiharaParams
from dolfinx_external_operator_amd._lib import declared_symbols


def _golden_embedded(golden):
    g = golden("isihara_analytic.npz")
    return g, H3.embed_plane_strain(g["F"])


def test_plane_strain_embedding_reproduces_the_reference_data(golden):
    """In-plane P and dP of the 3-D energy at [[F_2, 0], [0, 1]] are the golden's to 1e-13 of the scale (measured 6.4e-16, 4.7e-16);
    the out-of-plane shear stresses are exactly 0."""
    g, F = _golden_embedded(golden)
    P, dP = H3.reference(F)
    ip = H3.IN_PLANE
    eP, eD = H3.rel_err(P[:, ip], g["P"]), H3.rel_err(dP[:, ip][:, :, ip], g["dP"])
    print(f"in-plane P {eP:.2e}, dP {eD:.2e}")
    assert eP <= 1e-13 and eD <= 1e-13
    assert np.all(P[:, H3.SHEAR_OUT] == 0.0)


def test_identity_is_stress_free():
    P, dP = H3.reference(H3.EYE[None, :])
    assert np.all(P == 0.0)
    assert np.isfinite(dP).all()


def test_tangent_is_symmetric_and_forward_equals_reverse():
    F = H3.samples(300)
    _, dP = H3.reference(F)
    scale = np.abs(dP).max()
    sym = np.abs(dP - dP.transpose(0, 2, 1)).max() / scale
    rev = np.abs(dP - H3.reference_reverse(F)).max() / scale
    print(f"symmetry {sym:.2e}, forward against reverse {rev:.2e}")
    assert sym <= 1e-13 and rev <= 1e-13


def test_stress_is_objective():
    """P(Q F) = Q P(F) for a rotation Q"""
    rng = np.random.Generator(np.random.PCG64(3))
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    F = H3.samples(200).reshape(-1, 3, 3)
    P, _ = H3.reference(F)
    PQ, _ = H3.reference(np.einsum("ij,njk->nik", Q, F))
    want = np.einsum("ij,njk->nik", Q, P.reshape(-1, 3, 3)).reshape(-1, 9)
    assert H3.rel_err(PQ, want) <= 1e-13


def test_sample_generators_stay_in_the_model_range():
    assert H3.det_rows(H3.small_strain(1200)).min() > 0.5
    assert H3.det_rows(H3.large_stretch(600)).min() > 0.2
    assert H3.samples(1000).shape == (1000, 9) and H3.samples(1).shape == (1, 9)


def test_entry_points_exist_and_answer_as_their_2d_twins_without_a_context(hip_library):
    lib = hip_library
    for name in ("dxo_isihara3", "dxo_isihara3_field"):
        assert name in declared_symbols() and hasattr(lib, name)
    assert lib.dxo_abi_version() == 2
    prm = IsiharaParams(0.5, 1.0, 1.0, 1.5)
    buf = np.zeros(512)
    base = (buf.ctypes.data + 15) & ~15
    b = types.SimpleNamespace(prm=C.byref(prm), F=base, dP=base + 1024, P=base + 2048, u=base, mesh=None)
    for name, args in H3.plain_bad_calls(b):
        rc2, rc3 = lib.dxo_isihara(None, *args), lib.dxo_isihara3(None, *args)
        assert rc3 == rc2 == -1, name
    for name, args in H3.field_bad_calls(b):
        rc2, rc3 = lib.dxo_isihara_field(None, *args), lib.dxo_isihara3_field(None, *args)
        assert rc3 == rc2 == -1, name


# ------------------------------------------------------------------------- the long-double reference of oracle/hyper3_reference.py
# What tests/test_hyper3_reference_gpu.py holds the kernels to, and the constants of tests/hyper3_reference_cases.py: the reference
# against autograd, against mpmath at 50 digits, its mag, its symmetry, and C_REF measured on the float64 twin.
import pytest  # noqa: E402

import hyper3_reference_cases as RC  # noqa: E402
import icnn3_cases as I3  # noqa: E402
from oracle.hyper3_reference import LD, icnn3_ref, isihara3_ref  # noqa: E402

SETS = list(RC.sample_sets())
MODELS = ("isihara3", "icnn3")


def _twin(model, name):
    F = RC.sample_sets()[name]
    return isihara3_ref(F, H3.DEFAULTS, dtype=np.float64) if model == "isihara3" else icnn3_ref(F, RC.weights(), dtype=np.float64)


@pytest.fixture(scope="module")
def twin_ratios():
    """{(key of C_REF, set): ratio of the float64 twin}, the fp32 keys: the float32-network route against the long-double network"""
    out = {}
    for name in SETS:
        for model in MODELS:
            P, dP, mP, mdP = RC.reference(model, name)
            P6, dP6, _, _ = _twin(model, name)
            key = "isihara3" if model == "isihara3" else "icnn3 fp64"
            out[key + " P", name] = RC.worst_entry(P6, P, mP, RC.EPS64)[0]
            out[key + " dP", name] = RC.worst_entry(dP6, dP, mdP, RC.EPS64)[0]
        P3, dP3, _, _ = icnn3_ref(RC.sample_sets()[name], RC.weights(), net="fp32")
        out["icnn3 fp32 P", name] = RC.worst_entry(P3, P, mP, RC.EPS32)[0]
        out["icnn3 fp32 dP", name] = RC.worst_entry(dP3, dP, mdP, RC.EPS32)[0]
    return out


def test_float64_twin_stays_within_c_ref_and_c_ref_is_not_loose(twin_ratios):
    """Every figure of hyper3_reference_cases.C_REF holds on every sample set, and on the worst set the twin reaches more than a
    quarter of it: a constant can neither be too small nor silently loose."""
    for key, c in RC.C_REF.items():
        per_set = {name: twin_ratios[key, name] for name in SETS}
        worst = max(per_set, key=per_set.get)
        print(f"{key:14s} C_REF {c:5.1f}: worst {per_set[worst]:6.2f} on '{worst}'; " + ", ".join(f"{v:.2f}" for v in per_set.values()))
        assert per_set[worst] <= c, (key, worst, per_set[worst])
        assert per_set[worst] > c / 4, (key, per_set[worst])


@pytest.mark.parametrize("name", SETS)
def test_reference_matches_autograd_to_what_float64_allows(name):
    """torch autograd in float64 on the energy (forward over reverse, and reverse over reverse; the network as one function of F) is a
    float64 evaluation like any other: per entry within MARGIN * C_REF * 2^-53 * mag of the reference, what the kernels are allowed."""
    F = RC.sample_sets()[name]
    P, dP, mP, mdP = RC.reference("isihara3", name)
    Pa, dPa = H3.reference(F.copy())
    got = {"P": RC.worst_entry(Pa, P, mP, RC.EPS64), "dP": RC.worst_entry(dPa, dP, mdP, RC.EPS64),
           "dP reverse": RC.worst_entry(H3.reference_reverse(F.copy()), dP, mdP, RC.EPS64)}
    print("isihara3", got)
    assert got["P"][0] <= RC.MARGIN * RC.C_REF["isihara3 P"]
    assert max(got["dP"][0], got["dP reverse"][0]) <= RC.MARGIN * RC.C_REF["isihara3 dP"]
    P, dP, mP, mdP = RC.reference("icnn3", name)
    dPa, Pa = I3.autograd_stress_tangent(F.copy(), RC.weights())
    dPj, Pj = I3.icnn3_stress_tangent(F, RC.weights(), net_dtype=np.float64)
    got = {"P": RC.worst_entry(Pa, P, mP, RC.EPS64), "dP": RC.worst_entry(dPa, dP, mdP, RC.EPS64),
           "jets P": RC.worst_entry(Pj, P, mP, RC.EPS64), "jets dP": RC.worst_entry(dPj, dP, mdP, RC.EPS64)}
    print("icnn3", got)
    assert max(got["P"][0], got["jets P"][0]) <= RC.MARGIN * RC.C_REF["icnn3 fp64 P"]
    assert max(got["dP"][0], got["jets dP"][0]) <= RC.MARGIN * RC.C_REF["icnn3 fp64 dP"]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", SETS)
def test_mag_dominates_and_the_tangent_is_symmetric(model, name):
    """mag >= |ref| in every entry; mag = 0 only where every term vanishes, and then ref is an exact zero: on the dense sets mag > 0
    everywhere, on the plane-strain set it is 0 exactly in the entries that couple an out-of-plane shear to the plane; dP is built
    symmetric."""
    P, dP, mP, mdP = RC.reference(model, name)
    assert np.all((mP >= np.abs(P)) | np.isnan(P)) and np.all((mdP >= np.abs(dP)) | np.isnan(dP))
    assert np.all(P[mP == 0] == 0) and np.all(dP[mdP == 0] == 0)
    assert np.array_equal(dP, dP.transpose(0, 2, 1), equal_nan=True) and np.array_equal(mdP, mdP.transpose(0, 2, 1))
    if name == "inverted rows":
        bad = np.arange(P.shape[0]) % 3 == 1
        assert np.array_equal(np.isnan(P), np.broadcast_to((bad & (model == "isihara3"))[:, None], P.shape))
        assert np.array_equal(np.isnan(dP), np.broadcast_to((bad & (model == "isihara3"))[:, None, None], dP.shape))
    F = RC.sample_sets()[name]
    if np.all(F != 0):
        assert np.all(mP > 0) and np.all(mdP > 0)
    if name == "plane strain":
        out, inp, diag = H3.SHEAR_OUT, np.array([0, 1, 3, 4, 8]), np.array([0, 4, 8])
        assert np.all(mP[:, out] == 0) and np.all(mP[:, diag] > 0)
        assert np.all(mdP[:, out][:, :, inp] == 0) and np.all(mdP[:, diag][:, :, diag] > 0)


def test_nonpositive_determinant_is_nan_in_all_ninety_outputs_of_the_analytic_model():
    F = I3.inverted(5)
    F[3] = [1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 1.0, 1.0]                     # det F = 0
    F[4] = H3.EYE
    for dtype in (LD, np.float64):
        P, dP, mP, mdP = isihara3_ref(F, H3.DEFAULTS, dtype=dtype)
        assert np.isnan(P[:4]).all() and np.isnan(dP[:4]).all()
        assert np.isfinite(P[4]).all() and np.isfinite(dP[4]).all() and np.all(P[4] == 0)
    P, dP, _, _ = icnn3_ref(F[[0, 1, 2, 4]], RC.weights())                  # the network takes J = |det F|
    assert np.isfinite(P).all() and np.isfinite(dP).all()


# ---- mpmath at 50 digits
def _mp(x):
    """a long double as an mpf, exactly"""
    import mpmath as mp

    return mp.mpf(float(x)) + mp.mpf(float(x - LD(float(x))))


def _ld(x):
    """an mpf rounded to long double"""
    import mpmath as mp

    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def _mp_features(f):
    import mpmath as mp

    F = mp.matrix(3, 3)
    for i in range(9):
        F[i // 3, i % 3] = f[i]
    C = F.T * F
    CC = C * C
    I1 = C[0, 0] + C[1, 1] + C[2, 2]
    I2 = (I1 ** 2 - (CC[0, 0] + CC[1, 1] + CC[2, 2])) / 2
    J = abs(mp.det(F))
    return [I1 * J ** (mp.mpf(-2) / 3) - 3, I2 * J ** (mp.mpf(-4) / 3) - 3, (J - 1) ** 2]


def _mp_isihara(*f):
    import mpmath as mp

    c1, c2, c3, c4 = (mp.mpf(x) for x in H3.DEFAULTS)
    K = _mp_features(f)
    return c1 * K[0] + c2 * K[1] + c3 * K[0] ** 2 + c4 * K[2]


def _mp_network():
    """ICNN.forward as icnn3_cases.network_energy_torch states it, on mpf: x (3) -> y"""
    import mpmath as mp

    sp = lambda x: x if x > 20 else mp.log1p(mp.exp(x))                      # noqa: E731  (torch's softplus, threshold 20)
    w = {k: mp.matrix(np.atleast_2d(v).astype(np.float64).tolist()) for k, v in RC.weights().items()}
    col = lambda M: M.T if M.rows == 1 and M.cols > 1 else M                 # noqa: E731
    W = {layer: w[f"layers__{layer}__weights"].apply(sp) for layer in (1, 2, 3)}
    S3 = w["skip_layers__3__weights"].apply(sp)

    def net(*k):
        x = mp.matrix(list(k))
        z = w["layers__0__weight"] * x + col(w["layers__0__bias"])
        for layer in (1, 2):
            a = W[layer] * z + w[f"skip_layers__{layer}__weight"] * x + col(w[f"skip_layers__{layer}__bias"])
            z = a.apply(lambda t: sp(t) ** 2 / 12)
        return (W[3] * z + S3 * x)[0]
    return net


def _mp_points():
    """two points from each hard set, two rotations and two large stretches"""
    sets = RC.sample_sets()
    return [(name, i) for name in RC.HARD_SETS + ("rotations", "large stretch") for i in (0, sets[name].shape[0] - 1)]


def _unit(k, l=None):                                                        # noqa: E741
    e = [0] * 9
    e[k] += 1
    if l is not None:
        e[l] += 1
    return e


def test_analytic_reference_matches_mpmath_at_fifty_digits():
    """P = dW/dF and dP = d2W/dF2 by mpmath.diff of the energy as the docstring of hyper3_cases.py states it, at 12 points, all 9 + 45
    entries: within 8 * 2^-64 * mag."""
    import mpmath as mp

    pts = _mp_points()
    assert len(pts) == 12
    tol, worst = 8 * 2.0 ** -64, [0.0, 0.0]
    with mp.workdps(50):
        for name, i in pts:
            P, dP, mP, mdP = (a[i] for a in RC.reference("isihara3", name))
            f = [mp.mpf(float(x)) for x in RC.sample_sets()[name][i]]
            for k in range(9):
                worst[0] = max(worst[0], float(abs(mp.diff(_mp_isihara, f, _unit(k)) - _mp(P[k])) / (tol * _mp(mP[k]))))
                for l in range(k, 9):                                        # noqa: E741
                    worst[1] = max(worst[1], float(abs(mp.diff(_mp_isihara, f, _unit(k, l)) - _mp(dP[k, l])) / (tol * _mp(mdP[k, l]))))
    print(f"isihara3: worst |ref - mpmath| / (8 * 2^-64 * mag): P {worst[0]:.3f}, dP {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_network_reference_matches_mpmath_at_fifty_digits():
    """The network operator in two steps, at the same 12 points.

    1. Features, chain rule and H correction. The reference is given the network's gradient and Hessian by mpmath (mpmath.diff of the
       network in its three inputs, rounded to long double) in the place of its own, and compared with mpmath.diff of the whole energy
       ICNN(K(F)) in F: all 9 stresses at every point, the tangent rows 0, 4 and 8 (24 entries) at the first point of each hard set
       (a second derivative of the whole energy costs 70000 products at 50 digits). Within 8 * 2^-64 * mag.
    2. The network's own long-double rounding, which mag does not contain: mag carries |y_k|, |y_kl|, while a neuron's pre-activation
       is a sum of 64 signed terms, so the gradient in long double is off by some hundred units of 2^-64 |y_k| however the chain rule
       is written (measured: up to 270 in P). What the reference needs is to be well below what it judges: the long-double reference
       with its own network stays within 2^-55 * mag of mpmath, a quarter of one float64 rounding and 2 % of the smallest network
       C_REF; the figure is not taken from the measurement but from that purpose."""
    import mpmath as mp

    net, sets, w = _mp_network(), RC.sample_sets(), RC.weights()
    orders = [(k, l) for k in range(3) for l in range(k, 3)]
    cache = {}

    def mp_jets(x):
        dy, d2y = np.zeros(x.shape, dtype=LD), np.zeros(x.shape + (3,), dtype=LD)
        for p, row in enumerate(x):
            key = tuple(float(v) for v in row)
            if key not in cache:
                k = [_mp(v) for v in row]
                g = [_ld(mp.diff(net, k, [int(a == b) for b in range(3)])) for a in range(3)]
                h = {kl: _ld(mp.diff(net, k, [int(a == kl[0]) + int(a == kl[1]) for a in range(3)])) for kl in orders}
                cache[key] = (g, h)
            g, h = cache[key]
            dy[p] = g
            for (k_, l_), v in h.items():
                d2y[p, k_, l_] = d2y[p, l_, k_] = v
        return dy, d2y

    def energy(*f):
        return net(*_mp_features(f))

    tol, own = 8 * 2.0 ** -64, 2.0 ** -55
    worst = {"P": 0.0, "dP": 0.0, "own P": 0.0, "own dP": 0.0}
    with mp.workdps(50):
        for name, i in _mp_points():
            F = sets[name][i:i + 1]
            f = [mp.mpf(float(x)) for x in F[0]]
            P, dP, mP, mdP = (a[0] for a in icnn3_ref(F, w, net=mp_jets))
            Po, dPo, _, _ = (a[i] for a in RC.reference("icnn3", name))
            rows = (0, 4, 8) if i == 0 and name in RC.HARD_SETS else ()
            for k in range(9):
                exact = mp.diff(energy, f, _unit(k))
                worst["P"] = max(worst["P"], float(abs(exact - _mp(P[k])) / (tol * _mp(mP[k]))))
                worst["own P"] = max(worst["own P"], float(abs(exact - _mp(Po[k])) / (own * _mp(mP[k]))))
            for k in rows:
                for l in range(k, 9):                                        # noqa: E741
                    exact = mp.diff(energy, f, _unit(k, l))
                    worst["dP"] = max(worst["dP"], float(abs(exact - _mp(dP[k, l])) / (tol * _mp(mdP[k, l]))))
                    worst["own dP"] = max(worst["own dP"], float(abs(exact - _mp(dPo[k, l])) / (own * _mp(mdP[k, l]))))
    print("icnn3: |ref - mpmath| with mpmath's network derivatives, in units of 8 * 2^-64 * mag: "
          f"P {worst['P']:.3f}, dP {worst['dP']:.3f}; with its own, in units of 2^-55 * mag: P {worst['own P']:.3f}, dP {worst['own dP']:.3f}")
    assert worst["P"] <= 1.0 and worst["dP"] <= 1.0
    assert worst["own P"] <= 1.0 and worst["own dP"] <= 1.0


def test_the_meshes_cover_both_parities_and_three_pass_lengths():
    """what the fused cases run, from num_cells, nq and 64 // nq alone: pass lengths 16, 14 and 13; on every odd-group mesh at least
    three groups with both parities, and a partial last group on all but the one whose 72 cells are 8 full groups"""
    pps = {name: RC.pass_points(RC.fused_mesh(name))[0] for name in RC.FUSED_MESHES}
    print(pps)
    assert set(pps.values()) == {16, 14, 13}
    partial = []
    for name in RC.ODD_GROUP_MESHES:
        m = RC.fused_mesh(name)
        cpw = 64 // m.nq
        assert m.num_cells >= 2 * cpw + 1 and (cpw * m.nq) % 2 == 1
        partial.append(m.num_cells % cpw != 0)
    assert sum(partial) >= len(partial) - 1
