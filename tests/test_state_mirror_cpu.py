"""Host-side bookkeeping of make_von_mises(state="resident") and make_mohr_coulomb(state="resident") without a GPU: `_StateMirror`
and `_McMirror` against recording stand-ins for `_lib.VmState` / `_lib.McState` — when the holders are uploaded, when they are not,
what commit_state / state_changed do, and the sampled tripwire. The device side of the same protocol is tests/test_vm_state_gpu.py
and tests/test_return_map_entries_gpu.py."""
import warnings

import numpy as np
import pytest

from dolfinx_external_operator_amd.operators import _McMirror, _StateMirror


class _FakeState:
    """Stand-in for VmState (shape = (d, n), uploads of (sigma_n, p)) and McState (shape = (n,), uploads of (sigma_n,))."""

    def __init__(self, ctx, *shape):
        self.ctx, self.n = ctx, shape[-1]
        if len(shape) == 2:
            self.d = shape[0]
        self.uploads, self.commits, self.closed = [], 0, False

    def upload(self, *arrays):
        self.uploads.append(tuple(a.copy() for a in arrays))

    def commit(self):
        self.commits += 1

    def close(self):
        self.closed = True


class _FakeCtx:
    def __init__(self):
        self.states = []

    def vm_state(self, d, n):
        self.states.append(_FakeState(self, d, n))
        return self.states[-1]

    def mc_state(self, n):
        self.states.append(_FakeState(self, n))
        return self.states[-1]


class _Form:
    """One return map's mirror: its constructor, the leading arguments of sync() and how many holders it has."""

    def __init__(self, name):
        self.name = name
        self.d = 6 if name == "vm" else 4

    def arrays(self, n, rng=None):
        """The holders of n points: (sigma_n, p) or (sigma_n,); zeros without a generator."""
        if rng is None:
            sigma_n, p = np.zeros(n * self.d), np.zeros(n)
        else:
            sigma_n, p = rng.normal(size=n * self.d), np.abs(rng.normal(size=n))
        return (sigma_n, p) if self.name == "vm" else (sigma_n,)

    def mirror(self, arrays):
        return _StateMirror(*arrays) if self.name == "vm" else _McMirror(*arrays)

    def sync(self, m, c, n, arrays):
        return m.sync(c, self.d, n, *arrays) if self.name == "vm" else m.sync(c, n, *arrays)


@pytest.fixture(params=["vm", "mc"])
def form(request):
    return _Form(request.param)


def test_upload_once_then_commit_then_tripwire(form):
    n = 10_000
    rng = np.random.Generator(np.random.PCG64(1))
    arrays = form.arrays(n, rng)
    sigma_n, last = arrays[0], arrays[-1]               # last: p (von Mises) or sigma_n itself (Mohr-Coulomb)
    c = _FakeCtx()
    m = form.mirror(arrays)
    m.commit()                                          # nothing on the device yet: a no-op, not an error
    st = form.sync(m, c, n, arrays)
    assert len(st.uploads) == 1 and len(c.states) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for _ in range(3):                              # Newton iterations of one load step: no traffic
            assert form.sync(m, c, n, arrays) is st
    assert len(st.uploads) == 1
    sigma_n *= 1.01                                     # the reference's load-step update on the host ...
    if last is not sigma_n:
        last += 0.5
    m.commit()                                          # ... announced: device-side commit, no upload, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        form.sync(m, c, n, arrays)
        form.sync(m, c, n, arrays)
    assert st.commits == 1 and len(st.uploads) == 1
    sigma_n[::7] += 1.0                                 # changed behind the operator's back: tripwire -> warn + upload
    with pytest.warns(RuntimeWarning, match="re-uploading"):
        form.sync(m, c, n, arrays)
    assert len(st.uploads) == 2 and np.array_equal(st.uploads[-1][0], sigma_n)
    assert len(st.uploads[-1]) == len(arrays)
    last[5] = 9.0                                       # a single entry the samples may miss: announced by the caller
    m.invalidate()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        form.sync(m, c, n, arrays)
    assert len(st.uploads) == 3 and st.uploads[-1][-1][5] == 9.0


def test_a_new_batch_size_or_context_gets_a_new_mirror(form):
    c1, c2 = _FakeCtx(), _FakeCtx()
    small = form.arrays(100)
    m = form.mirror(small)
    s1 = form.sync(m, c1, 100, small)
    large = form.arrays(200)
    s2 = form.sync(m, c1, 200, large)
    assert s2 is not s1 and s1.closed and len(s2.uploads) == 1
    s3 = form.sync(m, c2, 200, large)
    assert s3 is not s2 and s2.closed and s3.ctx is c2 and len(s3.uploads) == 1
    with pytest.raises(RuntimeError, match="no call"):
        form.mirror(small).check()


def test_nan_state_does_not_trip_the_wire(form):
    arrays = form.arrays(100)
    arrays[0][:] = np.nan
    c = _FakeCtx()
    m = form.mirror(arrays)
    st = form.sync(m, c, 100, arrays)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        form.sync(m, c, 100, arrays)                     # NaN == NaN for the comparison of samples
    assert len(st.uploads) == 1
