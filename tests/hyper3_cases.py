"""Reference and sample points of the 3-D Isihara operator (dxo_isihara3): the energy
    W(F) = c1 (I1bar - 3) + c2 (I2bar - 3) + c3 (I1bar - 3)^2 + c4 (J - 1)^2,
    I1bar = J^(-2/3) I1, I2bar = J^(-4/3) I2, I1 = tr C, I2 = (I1^2 - tr C^2) / 2, C = F^T F, J = det F
in torch fp64, P = dW/dF by torch.func.grad and dP/dF by jacfwd of it. The determinant is written out by cofactors:
torch.linalg.det's second derivative (through its LU) returns NaN at some points (tests/golden/make_golden_isihara.py)."""
import functools

import numpy as np
import torch

DEFAULTS = (0.5, 1.0, 1.0, 1.5)


def det3(F):
    return (F[0, 0] * (F[1, 1] * F[2, 2] - F[1, 2] * F[2, 1]) - F[0, 1] * (F[1, 0] * F[2, 2] - F[1, 2] * F[2, 0])
            + F[0, 2] * (F[1, 0] * F[2, 1] - F[1, 1] * F[2, 0]))


def energy(Fv, c=DEFAULTS):
    F = Fv.reshape(3, 3)
    C = F.T @ F
    J = det3(F)
    I1 = torch.trace(C)
    I2 = 0.5 * (I1 ** 2 - torch.trace(C @ C))
    I1b = J ** (-2.0 / 3.0) * I1
    I2b = J ** (-4.0 / 3.0) * I2
    return c[0] * (I1b - 3.0) + c[1] * (I2b - 3.0) + c[2] * (I1b - 3.0) ** 2 + c[3] * (J - 1.0) ** 2


def reference(F, c=DEFAULTS):
    """(P[n][9], dP[n][9][9]) of F[n][9] (NumPy, fp64) by autograd on the energy."""
    Ft = torch.from_numpy(np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9))
    if Ft.shape[0] == 0:
        return np.empty((0, 9)), np.empty((0, 9, 9))
    grad = torch.func.grad(functools.partial(energy, c=c))
    P = torch.func.vmap(grad)(Ft)
    dP = torch.func.vmap(torch.func.jacfwd(grad))(Ft)
    return P.numpy(), dP.numpy()


def reference_reverse(F, c=DEFAULTS):
    """dP by reverse mode over the gradient: the cross-check of jacfwd."""
    Ft = torch.from_numpy(np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9))
    grad = torch.func.grad(functools.partial(energy, c=c))
    return torch.func.vmap(torch.func.jacrev(grad))(Ft).numpy()


def det_rows(F):
    F = np.asarray(F).reshape(-1, 3, 3)
    return np.linalg.det(F)


EYE = np.eye(3).reshape(9)


def fixed_points():
    """identity, a uniaxial stretch (isochoric), a simple shear, a pure dilation"""
    lam = 1.3
    return np.array([EYE,
                     np.diag([lam, lam ** -0.5, lam ** -0.5]).reshape(9),
                     (np.eye(3) + 0.4 * np.outer([1.0, 0, 0], [0, 1.0, 0])).reshape(9),
                     (0.8 * np.eye(3)).reshape(9)])


def small_strain(n, seed=7):
    """I + 0.1 N(0, 1): every one of the first 1200 points of the PCG64(7) draw has det F > 0.5"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return EYE + 0.1 * rng.normal(size=(n, 9))


def large_stretch(n, seed=11):
    """I + 0.3 N(0, 1) filtered to det F > 0.2"""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = EYE + 0.3 * rng.normal(size=(4 * n + 64, 9))
    F = F[det_rows(F) > 0.2][:n]
    assert F.shape[0] == n
    return F


def samples(n):
    """n points: the fixed ones first (as many as fit), then small strains and large stretches in halves"""
    fx = fixed_points()[:n]
    rest = n - fx.shape[0]
    a = rest // 2
    return np.ascontiguousarray(np.concatenate([fx, small_strain(a), large_stretch(rest - a)]))


def embed_plane_strain(F2):
    """F2[n][4] -> F[n][9] = [[F2, 0], [0, 1]]"""
    F2 = np.asarray(F2).reshape(-1, 2, 2)
    F = np.zeros((F2.shape[0], 3, 3))
    F[:, :2, :2] = F2
    F[:, 2, 2] = 1.0
    return F.reshape(-1, 9)


IN_PLANE = np.array([0, 1, 3, 4])          # entries of the 2x2 block in the row-major 3x3
SHEAR_OUT = np.array([2, 5, 6, 7])         # out-of-plane shears


def rel_err(a, b):
    """max |a - b| over the scale max |b|"""
    a, b = np.asarray(a), np.asarray(b)
    if b.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- bad-argument calls of dxo_isihara3 / dxo_isihara3_field and of their 2-D twins: (name, the arguments after the context), built
# from `b`: b.prm (byref of an IsiharaParams), b.F / b.dP / b.P / b.u (16-byte aligned addresses with room for 4 points), b.mesh (handle).
def plain_bad_calls(b):
    """[(name, args after ctx)] for dxo_isihara / dxo_isihara3 (ctx, prm, n, mem, F, dP, P)"""
    return [("NULL params", (None, 4, 0, b.F, b.dP, b.P)),
            ("n < 0", (b.prm, -1, 0, b.F, b.dP, b.P)),
            ("bad mem", (b.prm, 4, 7, b.F, b.dP, b.P)),
            ("NULL F", (b.prm, 4, 0, None, b.dP, b.P)),
            ("NULL dP", (b.prm, 4, 0, b.F, None, b.P)),
            ("NULL P", (b.prm, 4, 0, b.F, b.dP, None)),
            ("F off by 4 bytes", (b.prm, 4, 0, b.F + 4, b.dP, b.P)),
            ("host dP off by 4 bytes", (b.prm, 4, 0, b.F, b.dP + 4, b.P)),
            ("device P off by 8 bytes", (b.prm, 4, 1, b.F, b.dP, b.P + 8)),
            ("device F off by 8 bytes", (b.prm, 4, 1, b.F + 8, b.dP, b.P))]


def field_bad_calls(b):
    """[(name, args after ctx)] for dxo_isihara_field / dxo_isihara3_field (ctx, prm, mesh, mem, u, dP, P)"""
    return [("NULL params", (None, b.mesh, 0, b.u, b.dP, b.P)),
            ("NULL mesh", (b.prm, None, 0, b.u, b.dP, b.P)),
            ("bad mem", (b.prm, b.mesh, 7, b.u, b.dP, b.P)),
            ("NULL u", (b.prm, b.mesh, 0, None, b.dP, b.P)),
            ("NULL dP", (b.prm, b.mesh, 0, b.u, None, b.P)),
            ("NULL P", (b.prm, b.mesh, 0, b.u, b.dP, None)),
            ("u off by 4 bytes", (b.prm, b.mesh, 0, b.u + 4, b.dP, b.P)),
            ("device dP off by 8 bytes", (b.prm, b.mesh, 1, b.u, b.dP + 8, b.P)),
            ("device P off by 8 bytes", (b.prm, b.mesh, 1, b.u, b.dP, b.P + 8))]
