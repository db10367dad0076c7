"""Reference and sample points of the 3-D network operator (dxo_icnn3_eval): the ICNN of the hyperelasticity demo on the invariants
    K1 = I1 I3^(-1/3) - 3,  K2 = I2 I3^(-2/3) - 3,  K3 = (sqrt(I3) - 1)^2,  I1 = tr C, I2 = (I1^2 - tr C^2) / 2, I3 = (det F)^2
of a full 3x3 F. Two routes that share nothing but the weights:
  * the jets route: the feature map differentiated by torch.func in fp64, the network's value, gradient and Hessian in its input by
    oracle.icnn_oracle.network_jets (fp32 like the reference, or fp64), the chain rule and the H correction written out;
  * the whole network in torch fp64, differentiated as one function of F (grad, jacfwd of grad).
The determinant goes by cofactors (hyper3_cases.det3): torch.linalg.det's second derivative returns NaN at some points."""
import numpy as np
import torch

import hyper3_cases as H3
from oracle.icnn_oracle import network_jets

EYE3 = np.eye(3)


def features_torch(Fv):
    F = Fv.reshape(3, 3)
    C = F.T @ F
    t, s, D = torch.trace(C), torch.trace(C @ C), H3.det3(F)
    aD = torch.abs(D)                   # J = sqrt(I3) = |det F|, as the reference's features
    m = aD ** (-2.0 / 3.0)
    return torch.stack([m * t - 3.0, 0.5 * m * m * (t * t - s) - 3.0, (aD - 1.0) ** 2])


def features(F):
    """K (n, 3), dK/dF (n, 3, 9), d2K/dF2 (n, 3, 9, 9) of F (n, 9), fp64"""
    Ft = torch.from_numpy(np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9))
    K = torch.func.vmap(features_torch)(Ft)
    dK = torch.func.vmap(torch.func.jacrev(features_torch))(Ft)
    d2K = torch.func.vmap(torch.func.jacfwd(torch.func.jacrev(features_torch)))(Ft)
    return K.numpy(), dK.numpy(), d2K.numpy()


def correction_tangent(H):
    """d(F H)_(ia) / dF_(jc) = d_ij H_ca as a 9x9 matrix"""
    return np.einsum("ij,ca->iajc", EYE3, H).reshape(9, 9)


def h_correction(w, net_dtype=np.float32):
    """H = -P_NN(F = I) as a 3x3 matrix (demo_hyperelasticity.py:362-381). Analytically zero in 3-D: K is stationary at the identity."""
    K, dK, _ = features(H3.EYE[None])
    _, dy, _ = network_jets(K, w, net_dtype)
    return -np.einsum("nk,nki->ni", dy.astype(np.float64), dK)[0].reshape(3, 3)


def icnn3_stress_tangent(F, w, net_dtype=np.float32):
    """(dP (n, 9, 9), P (n, 9)) of F (n, 9): features and chain rule in fp64, the network in `net_dtype`"""
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
    if F.shape[0] == 0:
        return np.empty((0, 9, 9)), np.empty((0, 9))
    K, dK, d2K = features(F)
    _, dy, d2y = network_jets(K, w, net_dtype)
    dy, d2y = dy.astype(np.float64), d2y.astype(np.float64)
    H = h_correction(w, net_dtype)
    P = np.einsum("nk,nki->ni", dy, dK) + (F.reshape(-1, 3, 3) @ H).reshape(-1, 9)
    dP = np.einsum("nk,nkij->nij", dy, d2K) + np.einsum("nkl,nki,nlj->nij", d2y, dK, dK) + correction_tangent(H)[None]
    return dP, P


# ---- the second referee: the network as one torch function of F
def _torch_weights(w):
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in w.items()}


def network_energy_torch(x, wt):
    """ICNN.forward (:288-299) on the features x (3,), fp64"""
    sp = torch.nn.functional.softplus
    z = wt["layers__0__weight"] @ x + wt["layers__0__bias"]
    for layer in (1, 2):
        a = sp(wt[f"layers__{layer}__weights"]) @ z + wt[f"skip_layers__{layer}__weight"] @ x + wt[f"skip_layers__{layer}__bias"]
        z = sp(a) ** 2 / 12.0
    return (sp(wt["layers__3__weights"]) @ z + sp(wt["skip_layers__3__weights"]) @ x)[0]


def autograd_stress_tangent(F, w):
    """(dP, P) by differentiating the whole network energy in fp64; the H correction from the same route"""
    wt = _torch_weights(w)
    Ft = torch.from_numpy(np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9))

    def energy(Fv):
        return network_energy_torch(features_torch(Fv), wt)

    grad = torch.func.grad(energy)
    P = torch.func.vmap(grad)(Ft).numpy()
    dP = torch.func.vmap(torch.func.jacfwd(grad))(Ft).numpy()
    H = -grad(torch.from_numpy(H3.EYE.copy())).numpy().reshape(3, 3)
    return dP + correction_tangent(H)[None], P + (Ft.numpy().reshape(-1, 3, 3) @ H).reshape(-1, 9)


# ---- sample points
small_strain = H3.small_strain


def moderate(n, seed=13):
    """I + 0.3 N(0, 1) kept where 0.5 < det F < 2"""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = H3.EYE + 0.3 * rng.normal(size=(6 * n + 64, 9))
    d = H3.det_rows(F)
    F = F[(d > 0.5) & (d < 2.0)][:n]
    assert F.shape[0] == n
    return np.ascontiguousarray(F)


def inverted(n, seed=7):
    """small strains with F_00 lowered by 2.2: every point has det F < 0"""
    F = H3.small_strain(n, seed).copy()
    F[:, 0] -= 2.2
    assert H3.det_rows(F).max() < 0.0
    return F


def state_dict(w):
    return {k.replace("__", "."): v for k, v in w.items()}
