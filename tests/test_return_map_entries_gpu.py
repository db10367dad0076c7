"""The entry points of the two return maps against each other, at sizes that reach every branch of their host side.

von Mises and Mohr-Coulomb each have a plain entry (history variables passed with every call) and a `_state` entry (history
variables resident in a dxo_vm_state / dxo_mc_state). On the same values the two must agree BIT FOR BIT, before and after a commit,
host arrays and device arrays, copy mode and host-rebuild mode, with every combination of optional outputs. The pipeline's thresholds
are lowered through the options to their floors (64 points: dxo_ctx_set_option refuses less for host_chunk_points and
vm_rebuild_chunk_points; vm_rebuild_min_points has no floor), so a few hundred points span three chunks and a ragged fourth. The
refusals of both families are checked through the C entry points: return code, and a message that starts with the entry point's name.
Nothing here launches a kernel on a refused call."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from conftest import mc_tracing_inputs, vm_indeterminate_sigma0, vm_inputs
from dolfinx_external_operator_amd import MEM_DEVICE, MEM_HOST, Context, DeviceMesh, McParams, VmParams
from tools.synthetic import structured_mesh

pytestmark = pytest.mark.gpu

E, NU = 70e3, 0.3
H = E * (E / 100.0) / (E - E / 100.0)
CHUNK = 64                      # the floor of host_chunk_points and vm_rebuild_chunk_points
N3 = 3 * CHUNK + 37             # three whole chunks and a ragged one
SIZES = [0, 1, 777, N3]
E_NULL, E_DIM, E_SIZE, E_MEM, E_ALIGN = -1, -2, -3, -4, -5
MC_PRM = McParams(6778.0, 0.25, 3.45, np.pi / 6, np.pi / 6, 26 * np.pi / 180, 0.26 * 3.45 / np.tan(np.pi / 6), 1e-8, 200, 0)


@contextlib.contextmanager
def lowered_thresholds(ctx, rebuild=0):
    keys = ("vm_rebuild_min_points", "host_chunk_points", "vm_rebuild_chunk_points", "vm_host_tangent")
    saved = {k: ctx.get_option(k) for k in keys}
    try:
        for k, v in zip(keys, (0, CHUNK, CHUNK, int(rebuild))):
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            ctx.set_option(k, v)


def assert_same_bits(got, want, what):
    """uint64 / int32 views: NaN tangents (the 0/0 point) compare by bit pattern."""
    for g, w, name in zip(got, want, what):
        g, w = np.ascontiguousarray(g).reshape(-1), np.ascontiguousarray(w).reshape(-1)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        view = np.uint64 if g.dtype == np.float64 else np.int32
        np.testing.assert_array_equal(g.view(view), w.view(view), err_msg=name)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def dev_empty(n, dtype=None):
    import torch

    return torch.full((n,), -7, dtype=dtype or torch.float64, device="cuda:0")


def ptr(t):
    return None if t is None else t.data_ptr()


def on_torch_stream(ctx):
    import torch

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def sync():
    import torch

    torch.cuda.synchronize()


def fetch(ctx, address, n):
    out = np.empty(n)
    if n:
        ctx.copy(out, address, out.nbytes, 1)
    return out


# ------------------------------------------------------------------------------------------------------------ von Mises, points
@pytest.fixture(scope="module")
def vm_case(ctx):
    """(prm, deps, sigma_n, p) per d: seeded elastic and plastic points with the exact f_elastic == 0 state at the points 0 and 70."""
    made = {}

    def make(d):
        if d not in made:
            def evaluate(deps, sn, p, sigma_0):
                C_, s_, dp_ = np.empty(d * d), np.empty(d), np.empty(1)
                ctx.von_mises(VmParams(E, NU, sigma_0, H), d, 1, MEM_HOST, deps, sn, p, C_, s_, dp_)
                return C_, s_, dp_

            sigma_0, sn_row = vm_indeterminate_sigma0(evaluate, d)
            deps, sigma_n, p = vm_inputs(max(SIZES), d, seed=21 + d)
            for i in (0, 70):
                deps[i], sigma_n[i], p[i] = 0.0, sn_row, 0.0
            made[d] = (VmParams(E, NU, sigma_0, H), deps, sigma_n, p)
        return made[d]

    return make


def vm_plain(ctx, prm, d, n, mem, deps, sigma_n, p, tangent=True):
    if mem == MEM_HOST:
        C_, s, dp = np.full(n * d * d, -7.0), np.full(n * d, -7.0), np.full(n, -7.0)
        ctx.von_mises(prm, d, n, MEM_HOST, deps, sigma_n, p, C_, s, dp)
        return C_, s, dp
    t = [dev(a) for a in (deps, sigma_n, p)]
    C_, s, dp = dev_empty(n * d * d) if tangent else None, dev_empty(n * d), dev_empty(n)
    ctx.von_mises(prm, d, n, MEM_DEVICE, *(ptr(a) for a in t), ptr(C_), ptr(s), ptr(dp))
    sync()
    return None if C_ is None else C_.cpu().numpy(), s.cpu().numpy(), dp.cpu().numpy()


def vm_state_call(ctx, st, prm, d, n, mem, deps):
    """(C_tang, sigma, dp) of dxo_von_mises_state; on the device sigma = dp = NULL first (read back from the mirror), then given."""
    if mem == MEM_HOST:
        C_, s, dp = np.full(n * d * d, -7.0), np.full(n * d, -7.0), np.full(n, -7.0)
        st.call(prm, MEM_HOST, deps, C_, s, dp)
        return C_, s, dp
    t, C_ = dev(deps), dev_empty(n * d * d)
    st.call(prm, MEM_DEVICE, ptr(t), ptr(C_))
    sync()
    where = st.pointers()
    left = (C_.cpu().numpy(), fetch(ctx, where["sigma"], n * d), fetch(ctx, where["dp"], n))
    C2, s, dp = dev_empty(n * d * d), dev_empty(n * d), dev_empty(n)
    st.call(prm, MEM_DEVICE, ptr(t), ptr(C2), ptr(s), ptr(dp))
    sync()
    assert_same_bits((C2.cpu().numpy(), s.cpu().numpy(), dp.cpu().numpy()), left, ("C_tang", "sigma", "dp"))
    return left


@pytest.mark.parametrize("mem", [MEM_HOST, MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("rebuild", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [4, 6])
def test_von_mises_state_entry_equals_the_plain_entry(ctx, vm_case, d, n, rebuild, mem):
    prm, deps, sigma_n, p = vm_case(d)
    deps, sigma_n, p = deps[:n].copy(), sigma_n[:n].copy(), p[:n].copy()
    names = ("C_tang", "sigma", "dp")
    on_torch_stream(ctx)
    with lowered_thresholds(ctx, rebuild):
        want = vm_plain(ctx, prm, d, n, mem, deps, sigma_n, p)
        if n >= CHUNK:
            assert np.isnan(want[0].reshape(n, d * d)[[0, 70]]).all() and 0 < np.count_nonzero(want[2] > 0) < n   # 0/0, elastic, plastic
        if mem == MEM_DEVICE:     # the (sigma, dp)-only form of the plain entry: C_tang = NULL
            assert_same_bits(vm_plain(ctx, prm, d, n, mem, deps, sigma_n, p, tangent=False)[1:], want[1:], names[1:])
        st = ctx.vm_state(d, n)
        try:
            if mem == MEM_HOST:
                st.upload(sigma_n, p)
            else:
                held = dev(sigma_n), dev(p)
                st.upload(ptr(held[0]), ptr(held[1]), MEM_DEVICE)
            got = vm_state_call(ctx, st, prm, d, n, mem, deps)
            assert_same_bits(got, want, names)
            if n:
                st.commit()                                            # p += dp; sigma_n <- sigma on the device ...
                p += want[2]                                           # ... and on the host (demo_plasticity_von_mises.py:564-565)
                sigma_n[:] = want[1].reshape(n, d)
                assert_same_bits(vm_state_call(ctx, st, prm, d, n, mem, deps), vm_plain(ctx, prm, d, n, mem, deps, sigma_n, p), names)
        finally:
            st.close()


# ------------------------------------------------------------------------------------------------------------ von Mises, fields
@pytest.fixture(scope="module")
def small_meshes(ctx):
    """The smallest meshes the field kernels take: 6 x 5 boxes of P2 triangles (60 cells, 3 points each), 3 x 2 x 2 Q2 hexahedra with
    the 2 x 2 x 2 rule."""
    made = {}

    def make(cell):
        if cell not in made:
            m = structured_mesh(cell, (6, 5) if cell == "triangle" else (3, 2, 2), 2, distort=0.15, seed=3)
            made[cell] = (m, DeviceMesh.from_synthetic(m, ctx=ctx))
        return made[cell]

    yield make
    for _, dm in made.values():
        dm.close()


def field_plain(ctx, dm, prm, mem, u, sigma_n, p, n, d):
    if mem == MEM_HOST:
        C_, s, dp = np.full(n * d * d, -7.0), np.full(n * d, -7.0), np.full(n, -7.0)
        dm.von_mises(prm, u, sigma_n, p, C_, s, dp)
        return C_, s, dp
    t = [dev(a) for a in (u, sigma_n, p)]
    C_, s, dp = dev_empty(n * d * d), dev_empty(n * d), dev_empty(n)
    dm.von_mises(prm, *(ptr(a) for a in t), ptr(C_), ptr(s), ptr(dp), mem=MEM_DEVICE)
    sync()
    return C_.cpu().numpy(), s.cpu().numpy(), dp.cpu().numpy()


def field_state_call(ctx, st, dm, prm, mem, u, n, d):
    if mem == MEM_HOST:
        C_, s, dp = np.full(n * d * d, -7.0), np.full(n * d, -7.0), np.full(n, -7.0)
        st.call_field(prm, dm._h, MEM_HOST, u, C_, s, dp)
        return C_, s, dp
    t, C_ = dev(u), dev_empty(n * d * d)
    st.call_field(prm, dm._h, MEM_DEVICE, ptr(t), ptr(C_))           # sigma = dp = NULL: they stay in the mirror
    sync()
    where = st.pointers()
    return C_.cpu().numpy(), fetch(ctx, where["sigma"], n * d), fetch(ctx, where["dp"], n)


@pytest.mark.parametrize("mem", [MEM_HOST, MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("rebuild", [0, 1])
@pytest.mark.parametrize("cell", ["triangle", "hexahedron"])
def test_von_mises_field_state_entry_equals_the_plain_field_entry(ctx, small_meshes, cell, rebuild, mem):
    m, dm = small_meshes(cell)
    d, n = (4 if m.gdim == 2 else 6), m.num_cells * m.nq
    prm = VmParams(E, NU, 250.0, H)
    rng = np.random.Generator(np.random.PCG64(31))
    u = rng.normal(0.0, 1e-4, m.node_x.shape[0] * m.gdim)             # strains of about 1e-3 on cells this large, yield is near 5e-3 ...
    sigma_n, p = rng.normal(0.0, 150.0, (n, d)), np.abs(rng.normal(0.0, 1e-3, n))   # ... and the old stresses straddle sigma_0
    names = ("C_tang", "sigma", "dp")
    on_torch_stream(ctx)
    with lowered_thresholds(ctx, rebuild):
        want = field_plain(ctx, dm, prm, mem, u, sigma_n, p, n, d)
        assert 0 < np.count_nonzero(want[2] > 0) < n
        st = ctx.vm_state(d, n)
        try:
            st.upload(sigma_n, p)
            assert_same_bits(field_state_call(ctx, st, dm, prm, mem, u, n, d), want, names)
            st.commit()
            p += want[2]
            sigma_n[:] = want[1].reshape(n, d)
            assert_same_bits(field_state_call(ctx, st, dm, prm, mem, 1.5 * u, n, d), field_plain(ctx, dm, prm, mem, 1.5 * u, sigma_n, p, n, d), names)
        finally:
            st.close()


# ------------------------------------------------------------------------------------------------------------ Mohr-Coulomb
MC_NAMES = ("C_tang", "sigma", "niter", "yielding", "norm_res", "dlambda")
DIAGNOSTICS = {"all": (True, True, True, True), "none": (False, False, False, False), "niter+norm_res": (True, False, True, False)}


@pytest.fixture(scope="module")
def mc_case(oracle):
    return mc_tracing_inputs(oracle, max(SIZES), seed=77)


def mc_outputs(n, which, mem):
    """[C_tang, sigma, niter, yielding, norm_res, dlambda], None where an optional output is not asked for."""
    import torch

    sizes, ints = (16 * n, 4 * n, n, n, n, n), (False, False, True, False, False, False)
    wanted = (True, True) + tuple(which)
    if mem == MEM_HOST:
        return [None if not w else (np.full(k, -7, dtype=np.int32) if i else np.full(k, -7.0)) for k, i, w in zip(sizes, ints, wanted)]
    return [None if not w else dev_empty(k, torch.int32 if i else None) for k, i, w in zip(sizes, ints, wanted)]


def mc_host_view(outs):
    return [None if o is None else (o if isinstance(o, np.ndarray) else o.cpu().numpy()) for o in outs]


def mc_address(o):
    return o if o is None or isinstance(o, np.ndarray) else o.data_ptr()


def mc_plain(ctx, n, mem, deps, sigma_n, which):
    outs = mc_outputs(n, which, mem)
    ins = (deps, sigma_n) if mem == MEM_HOST else (dev(deps), dev(sigma_n))
    ctx.mohr_coulomb(MC_PRM, n, mem, *(mc_address(a) for a in ins), *(mc_address(o) for o in outs))
    sync()
    return mc_host_view(outs)


def mc_state_call(ctx, st, n, mem, deps, which):
    outs = mc_outputs(n, which, mem)
    t = deps if mem == MEM_HOST else dev(deps)
    st.call(MC_PRM, mem, mc_address(t), *(mc_address(o) for o in outs))
    sync()
    return mc_host_view(outs)


def assert_same_given(got, want):
    kept = [k for k, w in enumerate(want) if w is not None]
    assert [k for k, g in enumerate(got) if g is not None] == kept
    assert_same_bits([got[k] for k in kept], [want[k] for k in kept], [MC_NAMES[k] for k in kept])


@pytest.mark.parametrize("mem", [MEM_HOST, MEM_DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("diagnostics", list(DIAGNOSTICS))
@pytest.mark.parametrize("n", SIZES)
def test_mohr_coulomb_state_entry_equals_the_plain_entry(ctx, mc_case, n, diagnostics, mem):
    which = DIAGNOSTICS[diagnostics]
    deps, sigma_n = (np.ascontiguousarray(a[:n]) for a in mc_case)
    on_torch_stream(ctx)
    with lowered_thresholds(ctx):
        want = mc_plain(ctx, n, mem, deps, sigma_n, which)
        if n >= CHUNK and which[0]:
            assert 0 < np.count_nonzero(want[2] > 1) < n              # elastic points stop after one iteration, the yielding ones iterate
        st = ctx.mc_state(n)
        try:
            if mem == MEM_HOST:
                st.upload(sigma_n)
            else:
                held = dev(sigma_n)
                st.upload(ptr(held), MEM_DEVICE)
            assert_same_given(mc_state_call(ctx, st, n, mem, deps, which), want)
            if n:
                st.commit()                                            # sigma_n <- sigma (demo_plasticity_mohr_coulomb.py:728)
                assert_same_given(mc_state_call(ctx, st, n, mem, deps, which), mc_plain(ctx, n, mem, deps, want[1].reshape(n, 4), which))
        finally:
            st.close()


@pytest.mark.parametrize("diagnostics", list(DIAGNOSTICS))
def test_mohr_coulomb_field_equals_operand_then_point_entry(ctx, small_meshes, mc_case, diagnostics):
    which = DIAGNOSTICS[diagnostics]
    m, dm = small_meshes("triangle")
    n = m.num_cells * m.nq
    u = np.random.Generator(np.random.PCG64(32)).normal(0.0, 3e-4, m.node_x.shape[0] * 2)
    sigma_n = np.ascontiguousarray(mc_case[1][:n])
    with lowered_thresholds(ctx):
        got = mc_outputs(n, which, MEM_HOST)
        ctx.mohr_coulomb_field(MC_PRM, dm._h, MEM_HOST, u, sigma_n, *got)
        deps = dm.evaluate("eps", 2, u).reshape(n, 4)                  # dxo_eval_operand
        assert_same_given(got, mc_plain(ctx, n, MEM_HOST, deps, sigma_n, which))


# ------------------------------------------------------------------------------------------------------------ refusals
def _refusals():
    """(entry point, expected code, call(env) -> code). env: the library, the context handle, valid arrays of 8 points and states in
    the stages of their protocol. A pointer argument is an address or None."""
    nul = None
    bad_mem = 7
    cases = []

    def add(entry, code, call, note):
        cases.append(pytest.param(entry, code, call, id=f"{entry}-{note}"))

    # ---- von Mises
    add("dxo_vm_state_upload", E_NULL, lambda e: e.lib.dxo_vm_state_upload(e.h, nul, 0, e.sn6, e.p), "no-state")
    add("dxo_vm_state_download", E_NULL, lambda e: e.lib.dxo_vm_state_download(e.h, nul, 0, e.sn6, e.p), "no-state")
    add("dxo_vm_state_commit", E_NULL, lambda e: e.lib.dxo_vm_state_commit(e.h, nul), "no-state")
    add("dxo_vm_state_pointers", E_NULL, lambda e: e.lib.dxo_vm_state_pointers(e.h, nul, nul, nul, nul, nul), "no-state")
    add("dxo_von_mises_state", E_NULL, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, nul, 0, e.deps6, e.C6, e.s6, e.dp), "no-state")
    add("dxo_vm_state_upload", E_MEM, lambda e: e.lib.dxo_vm_state_upload(e.h, e.vm_fresh, bad_mem, e.sn6, e.p), "bad-mem")
    add("dxo_vm_state_download", E_MEM, lambda e: e.lib.dxo_vm_state_download(e.h, e.vm_up, bad_mem, e.sn6, e.p), "bad-mem")
    add("dxo_von_mises_state", E_MEM, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, e.vm_up, bad_mem, e.deps6, e.C6, e.s6, e.dp), "bad-mem")
    add("dxo_von_mises", E_MEM, lambda e: e.lib.dxo_von_mises(e.h, e.vm, 6, 8, bad_mem, e.deps6, e.sn6, e.p, e.C6, e.s6, e.dp), "bad-mem")
    add("dxo_vm_state_upload", E_NULL, lambda e: e.lib.dxo_vm_state_upload(e.h, e.vm_fresh, 0, e.sn6, nul), "no-array")
    add("dxo_von_mises_state", E_SIZE, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, e.vm_fresh, 0, e.deps6, e.C6, e.s6, e.dp), "before-upload")
    add("dxo_vm_state_download", E_SIZE, lambda e: e.lib.dxo_vm_state_download(e.h, e.vm_fresh, 0, e.sn6, e.p), "before-upload")
    add("dxo_vm_state_commit", E_SIZE, lambda e: e.lib.dxo_vm_state_commit(e.h, e.vm_up), "nothing-to-commit")
    add("dxo_vm_state_commit", 0, lambda e: e.lib.dxo_vm_state_commit(e.h, e.vm_empty), "empty-state")
    add("dxo_von_mises_state", E_NULL, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, e.vm_up, 0, e.deps6, e.C6, nul, e.dp), "host-no-sigma")
    add("dxo_von_mises_state", E_NULL, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, e.vm_up, 0, e.deps6, e.C6, e.s6, nul), "host-no-dp")
    add("dxo_von_mises_state", E_NULL, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, e.vm_up, 0, e.deps6, nul, e.s6, e.dp), "no-tangent")
    add("dxo_von_mises_state", E_ALIGN, lambda e: e.lib.dxo_von_mises_state(e.h, e.vm, e.vm_up, 0, e.deps6 + 4, e.C6, e.s6, e.dp), "off-by-4")
    add("dxo_von_mises", E_ALIGN, lambda e: e.lib.dxo_von_mises(e.h, e.vm, 6, 8, 0, e.deps6, e.sn6, e.p, e.C6, e.s6 + 4, e.dp), "off-by-4")
    add("dxo_von_mises", E_NULL, lambda e: e.lib.dxo_von_mises(e.h, e.vm, 6, 8, 0, e.deps6, e.sn6, e.p, nul, e.s6, e.dp), "host-no-tangent")
    add("dxo_von_mises", E_DIM, lambda e: e.lib.dxo_von_mises(e.h, e.vm, 5, 8, 0, e.deps6, e.sn6, e.p, e.C6, e.s6, e.dp), "d-5")
    add("dxo_vm_state_create", E_DIM, lambda e: e.lib.dxo_vm_state_create(e.h, 5, 8, C.byref(C.c_void_p())), "d-5")
    add("dxo_vm_state_create", E_SIZE, lambda e: e.lib.dxo_vm_state_create(e.h, 6, -1, C.byref(C.c_void_p())), "n-negative")
    add("dxo_von_mises_field_state", E_SIZE,
        lambda e: e.lib.dxo_von_mises_field_state(e.h, e.vm, e.mesh, e.vm_up, 0, e.u, e.C6, e.s6, e.dp), "state-of-another-shape")
    add("dxo_von_mises_field_state", E_SIZE,
        lambda e: e.lib.dxo_von_mises_field_state(e.h, e.vm, e.mesh, e.vm_mesh_fresh, 0, e.u, e.C6, e.s6, e.dp), "before-upload")
    add("dxo_von_mises_field_state", E_NULL,
        lambda e: e.lib.dxo_von_mises_field_state(e.h, e.vm, nul, e.vm_up, 0, e.u, e.C6, e.s6, e.dp), "no-mesh")
    add("dxo_von_mises_field", E_MEM,
        lambda e: e.lib.dxo_von_mises_field(e.h, e.vm, e.mesh, bad_mem, e.u, e.sn6, e.p, e.C6, e.s6, e.dp), "bad-mem")
    add("dxo_von_mises_field", E_ALIGN,
        lambda e: e.lib.dxo_von_mises_field(e.h, e.vm, e.mesh, 1, e.dev, e.dev + 8, e.dev, e.dev, e.dev, e.dev), "device-8-not-16")
    # ---- Mohr-Coulomb
    add("dxo_mc_state_upload", E_NULL, lambda e: e.lib.dxo_mc_state_upload(e.h, nul, 0, e.sn4), "no-state")
    add("dxo_mc_state_download", E_NULL, lambda e: e.lib.dxo_mc_state_download(e.h, nul, 0, e.sn4), "no-state")
    add("dxo_mc_state_commit", E_NULL, lambda e: e.lib.dxo_mc_state_commit(e.h, nul), "no-state")
    add("dxo_mc_state_pointers", E_NULL, lambda e: e.lib.dxo_mc_state_pointers(e.h, nul, nul, nul), "no-state")
    add("dxo_mohr_coulomb_state", E_NULL, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, nul, 0, e.deps4, e.C4, e.s4, e.it, e.y, e.y, e.y), "no-state")
    add("dxo_mc_state_upload", E_MEM, lambda e: e.lib.dxo_mc_state_upload(e.h, e.mc_fresh, bad_mem, e.sn4), "bad-mem")
    add("dxo_mc_state_download", E_MEM, lambda e: e.lib.dxo_mc_state_download(e.h, e.mc_up, bad_mem, e.sn4), "bad-mem")
    add("dxo_mohr_coulomb_state", E_MEM, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, e.mc_up, bad_mem, e.deps4, e.C4, e.s4, nul, nul, nul, nul), "bad-mem")
    add("dxo_mohr_coulomb", E_MEM, lambda e: e.lib.dxo_mohr_coulomb(e.h, e.mc, 8, bad_mem, e.deps4, e.sn4, e.C4, e.s4, nul, nul, nul, nul), "bad-mem")
    add("dxo_mc_state_upload", E_NULL, lambda e: e.lib.dxo_mc_state_upload(e.h, e.mc_fresh, 0, nul), "no-array")
    add("dxo_mohr_coulomb_state", E_SIZE, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, e.mc_fresh, 0, e.deps4, e.C4, e.s4, nul, nul, nul, nul), "before-upload")
    add("dxo_mc_state_download", E_SIZE, lambda e: e.lib.dxo_mc_state_download(e.h, e.mc_fresh, 0, e.sn4), "before-upload")
    add("dxo_mc_state_commit", E_SIZE, lambda e: e.lib.dxo_mc_state_commit(e.h, e.mc_up), "nothing-to-commit")
    add("dxo_mc_state_commit", 0, lambda e: e.lib.dxo_mc_state_commit(e.h, e.mc_empty), "empty-state")
    add("dxo_mohr_coulomb_state", E_NULL, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, e.mc_up, 0, e.deps4, e.C4, nul, nul, nul, nul, nul), "host-no-sigma")
    add("dxo_mohr_coulomb_state", E_ALIGN, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, e.mc_up, 0, e.deps4 + 4, e.C4, e.s4, nul, nul, nul, nul), "off-by-4")
    add("dxo_mohr_coulomb", E_ALIGN, lambda e: e.lib.dxo_mohr_coulomb(e.h, e.mc, 8, 0, e.deps4, e.sn4, e.C4, e.s4, nul, e.y + 4, nul, nul), "off-by-4")
    add("dxo_mohr_coulomb", E_ALIGN, lambda e: e.lib.dxo_mohr_coulomb(e.h, e.mc, 8, 1, e.dev, e.dev + 8, e.dev, e.dev, nul, nul, nul, nul), "device-8-not-16")
    add("dxo_mohr_coulomb_state", E_ALIGN, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, e.mc_up, 1, e.dev, e.dev + 8, e.dev, nul, nul, nul, nul), "device-8-not-16")
    add("dxo_mohr_coulomb_field", E_ALIGN,
        lambda e: e.lib.dxo_mohr_coulomb_field(e.h, e.mc, e.mesh, 1, e.dev, e.dev, e.dev, e.dev + 8, nul, nul, nul, nul), "device-8-not-16")
    add("dxo_mohr_coulomb", E_ALIGN, lambda e: e.lib.dxo_mohr_coulomb(e.h, e.mc, 8, 0, e.deps4, e.sn4, e.C4, e.s4, e.it + 2, nul, nul, nul), "niter-off-by-2")
    add("dxo_mohr_coulomb_state", E_ALIGN, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc, e.mc_up, 0, e.deps4, e.C4, e.s4, e.it + 2, nul, nul, nul), "niter-off-by-2")
    add("dxo_mohr_coulomb_field", E_ALIGN,
        lambda e: e.lib.dxo_mohr_coulomb_field(e.h, e.mc, e.mesh, 0, e.u, e.sn4, e.C4, e.s4, e.it + 2, nul, nul, nul), "niter-off-by-2")
    add("dxo_mohr_coulomb", E_SIZE, lambda e: e.lib.dxo_mohr_coulomb(e.h, e.mc_neg, 8, 0, e.deps4, e.sn4, e.C4, e.s4, nul, nul, nul, nul), "nitermax-negative")
    add("dxo_mohr_coulomb_state", E_SIZE, lambda e: e.lib.dxo_mohr_coulomb_state(e.h, e.mc_neg, e.mc_up, 0, e.deps4, e.C4, e.s4, nul, nul, nul, nul), "nitermax-negative")
    add("dxo_mohr_coulomb_field", E_SIZE,
        lambda e: e.lib.dxo_mohr_coulomb_field(e.h, e.mc_neg, e.mesh, 0, e.u, e.sn4, e.C4, e.s4, nul, nul, nul, nul), "nitermax-negative")
    add("dxo_mc_state_create", E_SIZE, lambda e: e.lib.dxo_mc_state_create(e.h, -1, C.byref(C.c_void_p())), "n-negative")
    return cases


class _Env:
    pass


@pytest.fixture(scope="module")
def refusal_env(ctx, small_meshes):
    """Everything a refused call is handed: real arrays (a refusal must come before any of them is touched), and states that are fresh
    (never uploaded), uploaded (no call yet) and empty (n = 0)."""
    import torch

    e = _Env()
    e.lib, e.h = ctx.lib, ctx._h
    m, dm = small_meshes("triangle")
    npts = m.num_cells * m.nq
    size = max(8, npts)                      # points every array covers: the 8 of the point calls, the mesh's of the field calls
    widths = {"deps6": 6, "sn6": 6, "p": 1, "C6": 36, "s6": 6, "dp": 1, "deps4": 4, "sn4": 4, "C4": 16, "s4": 4, "y": 1}
    keep = {k: np.zeros(size * w) for k, w in widths.items()}
    keep["u"] = np.zeros(m.node_x.shape[0] * 2)
    keep["it"] = np.zeros(size, dtype=np.int32)
    keep["dev"] = torch.zeros(64 * size, dtype=torch.float64, device="cuda:0")
    for k, a in keep.items():
        setattr(e, k, a.data_ptr() if k == "dev" else a.ctypes.data)
    e.vm, e.mc = C.byref(VmParams(E, NU, 250.0, H)), C.byref(MC_PRM)
    e.mc_neg = C.byref(McParams(6778.0, 0.25, 3.45, 0.5, 0.5, 0.45, 1.5, 1e-8, -1, 0))
    e.mesh = dm._h
    states = {"vm_fresh": ctx.vm_state(6, 8), "vm_up": ctx.vm_state(6, 8), "vm_empty": ctx.vm_state(6, 0), "vm_mesh_fresh": ctx.vm_state(4, npts),
              "mc_fresh": ctx.mc_state(8), "mc_up": ctx.mc_state(8), "mc_empty": ctx.mc_state(0)}
    states["vm_up"].upload(keep["sn6"], keep["p"])
    states["mc_up"].upload(keep["sn4"])
    for k, st in states.items():
        setattr(e, k, st._h)
    e.keep = (keep, states)
    yield e
    for st in states.values():
        st.close()


@pytest.mark.parametrize("entry,code,call", _refusals())
def test_refusals_name_their_entry_point(ctx, refusal_env, entry, code, call):
    assert call(refusal_env) == code
    if code:
        assert ctx.lib.dxo_last_error(ctx._h).decode().startswith(entry + ":")


@pytest.mark.parametrize("kind", ["vm", "mc"])
def test_destroy_after_the_context_is_closed_frees_the_block(hip_library, kind):
    """The finalizer of a state may run after its context is gone (ctx == NULL): the device block is still freed."""
    import torch

    n = 1 << 21
    block = (2 * 6 + 2) * 8 * n if kind == "vm" else 2 * 4 * 8 * n        # 224 MiB / 128 MiB: far above the allocator's granularity
    own = Context(0)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    st = own.vm_state(6, n) if kind == "vm" else own.mc_state(n)
    held = torch.cuda.mem_get_info(0)[0]
    own.close()
    assert own._h is None
    st.close()                                                            # dxo_*_state_destroy(NULL, state)
    after = torch.cuda.mem_get_info(0)[0]
    assert before - held >= 0.9 * block, (before, held, block)
    assert after - held >= 0.9 * block, (held, after, block)
