// mc3_core.h — the per-point Mohr-Coulomb (Abbo-Sloan) return mapping of mc_core.h on the six-component Mandel vector
// (xx, yy, zz, sqrt2 xy, sqrt2 xz, sqrt2 yz), with the same forward-mode-through-Newton tangent. Host/device compilable.
//
// The yield surface and the plastic potential are functions of the invariants I1, J2, J3 only, so everything mc_core.h does in
// (J2, J3) — the truncated Taylor type T23, lode_arg, F_taylor, lode_sin_cos, mc_rsqrt, mc_recip, Const / make_const — is used
// as it stands. What is written again here is the tensor algebra: dev, C, S = C^-1 on six components, J3 = det s with its
// gradient dev q(s) (q = Mandel vector of the cofactor of s) and its Hessian (the polarisation of the quadratic q), the dense
// symmetric 6x6 forms of hess(g) and T(t) = D_t hess(g) (21 numbers each), an unrolled 6x6 LDL^T, and the 7x6 tangent iterate
//     Y_{k+1} = J^-1 ( [C; 0] + (D J [Y_k]) t )        (the recursion documented at the top of mc_core.h).
// With s4 = s5 = 0 every expression below reduces to its plane-strain twin in mc_core.h.
#pragma once

#include "mc_core.h"

#if defined(__clang__)
#define MC3_UNROLL _Pragma("unroll")
#else
#define MC3_UNROLL
#endif

namespace mc3 {

using mc::Const;
using mc::LodeArg;
using mc::T23;

constexpr double RS2 = 0.70710678118654752440;   // 1 / sqrt 2

// ---- 6-vector helpers
DXO_HD void devv(const double* v, double* out) {  // dev @ v
    // no FMA contraction: a hydrostatic stress must give s == 0 exactly (then J2 == 0 and f is NaN, as in the reference)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double m = (v[0] + v[1] + v[2]) * (1.0 / 3.0);
    out[0] = v[0] - m;
    out[1] = v[1] - m;
    out[2] = v[2] - m;
    out[3] = v[3];
    out[4] = v[4];
    out[5] = v[5];
}
DXO_HD double dot6(const double* a, const double* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
DXO_HD void C_times(const Const& k, const double* x, double* out) {  // C_elas @ x: lmbda on the leading 3x3 block, 2 mu on the diagonal
    const double t = k.lmbda * (x[0] + x[1] + x[2]);
    out[0] = t + k.mu2 * x[0];
    out[1] = t + k.mu2 * x[1];
    out[2] = t + k.mu2 * x[2];
    out[3] = k.mu2 * x[3];
    out[4] = k.mu2 * x[4];
    out[5] = k.mu2 * x[5];
}
DXO_HD void S_times(const Const& k, const double* x, double* out) {  // C_elas^-1 @ x
    const double t = k.nu * (x[0] + x[1] + x[2]);
    out[0] = k.inv_E * ((1.0 + k.nu) * x[0] - t);
    out[1] = k.inv_E * ((1.0 + k.nu) * x[1] - t);
    out[2] = k.inv_E * ((1.0 + k.nu) * x[2] - t);
    out[3] = k.inv_E * (1.0 + k.nu) * x[3];
    out[4] = k.inv_E * (1.0 + k.nu) * x[4];
    out[5] = k.inv_E * (1.0 + k.nu) * x[5];
}
DXO_HD double det_s(const double* s) {   // J3 = det s; the first term is the plane-strain expression
    return s[2] * (s[0] * s[1] - s[3] * s[3] / 2.0) + s[3] * s[4] * s[5] * RS2 - 0.5 * (s[0] * s[5] * s[5] + s[1] * s[4] * s[4]);
}
DXO_HD void cof_s(const double* s, double* q) {   // Mandel vector of the cofactor of s = grad_s det s
    q[0] = s[1] * s[2] - s[5] * s[5] / 2.0;
    q[1] = s[0] * s[2] - s[4] * s[4] / 2.0;
    q[2] = s[0] * s[1] - s[3] * s[3] / 2.0;
    q[3] = s[4] * s[5] * RS2 - s[2] * s[3];
    q[4] = s[3] * s[5] * RS2 - s[1] * s[4];
    q[5] = s[3] * s[4] * RS2 - s[0] * s[5];
}
// hess_s J3 (s) applied to w = q(s + w) - q(s) - q(w), the polarisation of the quadratic cofactor; linear in s (so it also
// serves D_t hess J3 with s -> dev t)
DXO_HD void Qs_times(const double* s, const double* w, double* out) {
    out[0] = s[2] * w[1] + s[1] * w[2] - s[5] * w[5];
    out[1] = s[2] * w[0] + s[0] * w[2] - s[4] * w[4];
    out[2] = s[1] * w[0] + s[0] * w[1] - s[3] * w[3];
    out[3] = (s[4] * w[5] + s[5] * w[4]) * RS2 - s[3] * w[2] - s[2] * w[3];
    out[4] = (s[3] * w[5] + s[5] * w[3]) * RS2 - s[4] * w[1] - s[1] * w[4];
    out[5] = (s[3] * w[4] + s[4] * w[3]) * RS2 - s[5] * w[0] - s[0] * w[5];
}

struct Surf {
    double s[6], q[6];     // grad J2 = s, grad J3 = dev q(s)
    double I1;
    double f, g;
    T23 F[2];              // F for angle phi (f) and psi (g)
};

template <bool SAME>
DXO_HD void surf_eval(const Const& k, const double* sig, Surf& o) {
    devv(sig, o.s);
    o.I1 = sig[0] + sig[1] + sig[2];
    const double* s = o.s;
    const double J2 = 0.5 * dot6(s, s);
    const double J3 = det_s(s);
    double qs[6];
    cof_s(s, qs);
    devv(qs, o.q);
    LodeArg lode;
    mc::lode_arg(k, J2, J3, lode);
    o.F[1] = mc::F_taylor(k, 1, J2, lode);
    o.g = o.I1 / 3.0 * k.sin_a[1] + o.F[1].c[0] - k.c * k.cos_a[1];
    if constexpr (SAME) {
        o.f = o.g;
    } else {
        o.F[0] = mc::F_taylor(k, 0, J2, lode);
        o.f = o.I1 / 3.0 * k.sin_a[0] + o.F[0].c[0] - k.c * k.cos_a[0];
    }
}

DXO_HD void grad_surface(const Const& k, const Surf& e, int ia, double* out) {  // d surface / d sigma
    const double Fx = e.F[ia].c[1], Fy = e.F[ia].c[2];
    const double h = k.sin_a[ia] / 3.0;
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) out[i] = (i < 3 ? h : 0.0) + Fx * e.s[i] + Fy * e.q[i];
}

// ---- the literal chain-rule operators (the cross-check of the dense forms below; hess_apply also gives hess(f) t when phi != psi)
DXO_HD void hess_apply(const Surf& e, int ia, const double* v, double* out) {
    const double* F = e.F[ia].c;
    double Pv[6], Qv[6], tmp[6];
    devv(v, Pv);
    Qs_times(e.s, Pv, tmp);
    devv(tmp, Qv);
    const double al = dot6(e.s, v), be = dot6(e.q, v);
    const double cp = F[3] * al + F[4] * be, cq = F[4] * al + F[5] * be;
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) out[i] = F[1] * Pv[i] + F[2] * Qv[i] + cp * e.s[i] + cq * e.q[i];
}
struct Third {
    double Pt[6], Qt[6];
    double a, b;
    double dFx, dFy, dFxx, dFxy, dFyy;
};
DXO_HD void third_setup(const Surf& e, int ia, const double* t, Third& o) {
    const double* F = e.F[ia].c;
    double tmp[6];
    devv(t, o.Pt);
    Qs_times(e.s, o.Pt, tmp);
    devv(tmp, o.Qt);
    o.a = dot6(e.s, t);
    o.b = dot6(e.q, t);
    o.dFx = F[3] * o.a + F[4] * o.b;
    o.dFy = F[4] * o.a + F[5] * o.b;
    o.dFxx = F[6] * o.a + F[7] * o.b;
    o.dFxy = F[7] * o.a + F[8] * o.b;
    o.dFyy = F[8] * o.a + F[9] * o.b;
}
DXO_HD void third_apply(const Surf& e, int ia, const Third& T, const double* v, double* out) {   // T(t) v = D_t (H v)
    const double* F = e.F[ia].c;
    double Pv[6], Qv[6], Rv[6], tmp[6];
    devv(v, Pv);
    Qs_times(e.s, Pv, tmp);
    devv(tmp, Qv);
    Qs_times(T.Pt, Pv, tmp);
    devv(tmp, Rv);
    const double al = dot6(e.s, v), be = dot6(e.q, v);
    const double dal = dot6(T.Pt, v), dbe = dot6(T.Qt, v);
    const double cp = T.dFxx * al + F[3] * dal + T.dFxy * be + F[4] * dbe;
    const double cq = T.dFxy * al + F[4] * dal + T.dFyy * be + F[5] * dbe;
    const double ep = F[3] * al + F[4] * be, eq = F[4] * al + F[5] * be;
    MC3_UNROLL
    for (int i = 0; i < 6; ++i)
        out[i] = T.dFx * Pv[i] + T.dFy * Qv[i] + F[2] * Rv[i] + cp * e.s[i] + ep * T.Pt[i] + cq * e.q[i] + eq * T.Qt[i];
}

// ---- the same operators as dense symmetric 6x6 matrices: 21 numbers, upper triangle by rows
// (00 01 02 03 04 05 | 11 12 13 14 15 | 22 23 24 25 | 33 34 35 | 44 45 | 55)
struct Sym6 { double m[21]; };
constexpr int sidx(int i, int j) { return i <= j ? 6 * i - (i * (i - 1)) / 2 + (j - i) : 6 * j - (j * (j - 1)) / 2 + (i - j); }
DXO_HD void sym_apply(const Sym6& A, const double* v, double* out) {
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        double acc = A.m[sidx(i, 0)] * v[0];
        MC3_UNROLL
        for (int j = 1; j < 6; ++j) acc += A.m[sidx(i, j)] * v[j];
        out[i] = acc;
    }
}
// 3 B(s), B(s) = dev Q(s) dev for a deviatoric s (s0 + s1 + s2 = 0): the normal block and the xy column are those of mc_core.h
DXO_HD void dev_q_dev3(const double* s, double* B) {
    const double r3 = 3.0 * RS2;
    B[0] = 2.0 * s[0]; B[1] = 2.0 * s[2]; B[2] = 2.0 * s[1]; B[3] = s[3]; B[4] = s[4]; B[5] = -2.0 * s[5];
    B[6] = 2.0 * s[1]; B[7] = 2.0 * s[0]; B[8] = s[3]; B[9] = -2.0 * s[4]; B[10] = s[5];
    B[11] = 2.0 * s[2]; B[12] = -2.0 * s[3]; B[13] = s[4]; B[14] = s[5];
    B[15] = -3.0 * s[2]; B[16] = r3 * s[5]; B[17] = r3 * s[4];
    B[18] = -3.0 * s[1]; B[19] = r3 * s[3];
    B[20] = -3.0 * s[0];
}
DXO_HD void sym_add_outer2(Sym6& A, const double* x, const double* y, const double* z, const double* w) {
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        MC3_UNROLL
        for (int j = i; j < 6; ++j) A.m[sidx(i, j)] += x[i] * y[j] + z[i] * w[j];
    }
}
DXO_HD void sym_add_dev(Sym6& A, double c) {   // A += c dev
    const double d = c * (2.0 / 3.0), o = c * (-1.0 / 3.0);
    A.m[0] += d; A.m[1] += o; A.m[2] += o;
    A.m[6] += d; A.m[7] += o;
    A.m[11] += d;
    A.m[15] += c; A.m[18] += c; A.m[20] += c;
}
// hess(surface) dense; also returns a = Fxx s + Fxy q, b = Fxy s + Fyy q (third_dense needs them again)
DXO_HD void hess_dense(const Surf& e, int ia, Sym6& H, double* a, double* b) {
    const double* F = e.F[ia].c;
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        a[i] = F[3] * e.s[i] + F[4] * e.q[i];
        b[i] = F[4] * e.s[i] + F[5] * e.q[i];
    }
    double B[21];
    dev_q_dev3(e.s, B);
    const double fy3 = F[2] * (1.0 / 3.0);
    MC3_UNROLL
    for (int n = 0; n < 21; ++n) H.m[n] = fy3 * B[n];
    sym_add_dev(H, F[1]);
    sym_add_outer2(H, a, e.s, b, e.q);
}
// T(t) = D_t hess(surface) dense, for the direction t
DXO_HD void third_dense(const Surf& e, int ia, const double* t, const double* a, const double* b, Sym6& T) {
    const double* F = e.F[ia].c;
    double Pt[6], Qt[6], tmp[6];
    devv(t, Pt);
    Qs_times(e.s, Pt, tmp);   // dev Q(s) dev t
    devv(tmp, Qt);
    const double al = dot6(e.s, t), be = dot6(e.q, t);
    const double dFx = F[3] * al + F[4] * be, dFy = F[4] * al + F[5] * be;
    const double dFxx = F[6] * al + F[7] * be, dFxy = F[7] * al + F[8] * be, dFyy = F[8] * al + F[9] * be;
    double c1[6], c2[6];
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        c1[i] = dFxx * e.s[i] + dFxy * e.q[i] + F[3] * Pt[i] + F[4] * Qt[i];
        c2[i] = dFxy * e.s[i] + dFyy * e.q[i] + F[4] * Pt[i] + F[5] * Qt[i];
    }
    const double dfy3 = dFy * (1.0 / 3.0), fy3 = F[2] * (1.0 / 3.0);
    {
        double B[21], Bt[21];
        dev_q_dev3(e.s, B);
        dev_q_dev3(Pt, Bt);
        MC3_UNROLL
        for (int n = 0; n < 21; ++n) T.m[n] = dfy3 * B[n] + fy3 * Bt[n];
    }
    sym_add_dev(T, dFx);
    sym_add_outer2(T, e.s, c1, e.q, c2);
    sym_add_outer2(T, Pt, a, Qt, b);
}

// LDL^T of a symmetric 6x6, no pivoting, reciprocal pivots; l(i, j), i > j, at i (i - 1) / 2 + j
struct Ldl { double l[15]; double inv[6]; };
constexpr int lidx(int i, int j) { return (i * (i - 1)) / 2 + j; }
DXO_HD void ldl_factor(const Sym6& M, Ldl& f) {
    double d[6];
    MC3_UNROLL
    for (int j = 0; j < 6; ++j) {
        double w[6];
        double dj = M.m[sidx(j, j)];
        MC3_UNROLL
        for (int k = 0; k < j; ++k) {
            w[k] = f.l[lidx(j, k)] * d[k];
            dj -= f.l[lidx(j, k)] * w[k];
        }
        d[j] = dj;
        f.inv[j] = mc::mc_recip(dj);
        MC3_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double acc = M.m[sidx(j, i)];
            MC3_UNROLL
            for (int k = 0; k < j; ++k) acc -= f.l[lidx(i, k)] * w[k];
            f.l[lidx(i, j)] = acc * f.inv[j];
        }
    }
}
DXO_HD void ldl_solve(const Ldl& f, const double* b, double* x) {
    double z[6];
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        double acc = b[i];
        MC3_UNROLL
        for (int k = 0; k < i; ++k) acc -= f.l[lidx(i, k)] * z[k];
        z[i] = acc;
    }
    MC3_UNROLL
    for (int i = 5; i >= 0; --i) {
        double acc = z[i] * f.inv[i];
        MC3_UNROLL
        for (int k = i + 1; k < 6; ++k) acc -= f.l[lidx(k, i)] * x[k];
        x[i] = acc;
    }
}

struct Result {
    double sigma[6];
    double C_tang[36];  // row-major d sigma_i / d deps_j
    int32_t niter;
    double yielding, norm_res, dlambda;
};

DXO_HD double residual(const Const& k, const Surf& e, const double* sig, double dl, const double* deps, const double* sn,
                       const double* gradg, double* r_sig, double* r_f) {
    double de[6], Cd[6];
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) de[i] = deps[i] - dl * gradg[i];
    mc3::C_times(k, de, Cd);
    double acc = 0.0;
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        r_sig[i] = sig[i] - sn[i] - Cd[i];
        acc += r_sig[i] * r_sig[i];
    }
    *r_f = e.f;
    acc += e.f * e.f;
    return sqrt(acc);
}

// f(sigma) only — the trial-stress test; the value path of surf_eval / F_taylor (see mc::f_value for `ia`)
DXO_HD double f_value(const Const& k, const double* sig, int ia = 0) {
    double s[6];
    devv(sig, s);
    const double I1 = sig[0] + sig[1] + sig[2];
    const double J2 = 0.5 * dot6(s, s);
    const double J3 = det_s(s);
    const double y2 = mc::mc_rsqrt(J2);
    double arg = (-(3.0 * sqrt(3.0)) / 2.0) * J3 * ((y2 * y2) * y2);
    if (arg < -1.0 || arg > 1.0) arg = arg < 0.0 ? -1.0 : 1.0;
    double K;
    if (fabs(arg) > k.sin3T) {
        const bool neg = arg < 0.0;
        const double Ak = neg ? k.A[ia][0] : k.A[ia][1], Bk = neg ? k.B[ia][0] : k.B[ia][1], Ck = neg ? k.Cc[ia][0] : k.Cc[ia][1];
        K = Ak + Bk * arg + Ck * (arg * arg);
    } else {
        double sn, cs;
        const double x1 = (1.0 - arg) * (1.0 + arg);
        mc::lode_sin_cos(arg, x1 * mc::mc_rsqrt(x1), sn, cs);
        K = cs - k.k_lin[ia] * sn;
    }
    return I1 / 3.0 * k.sin_a[ia] + sqrt(J2 * (K * K) + k.ag2s2[ia]) - k.c * k.cos_a[ia];
}

DXO_HD double c_elas_entry(const Const& k, int i, int j) { return ((i < 3 && j < 3) ? k.lmbda : 0.0) + (i == j ? k.mu2 : 0.0); }

// Elastic branch: one iteration with J = I; deps == 0 gives 0/0 = NaN > tol false: ZERO iterations, sigma = sigma_n, C_tang = 0
DXO_HD void elastic_point(const Const& k, const double* sn, const double* Ce, const double* trial, Result& R) {
    const double n0 = sqrt(dot6(Ce, Ce));
    R.dlambda = 0.0;
    if (!(n0 / n0 > k.tol)) {
        for (int i = 0; i < 6; ++i) R.sigma[i] = sn[i];
        for (int i = 0; i < 36; ++i) R.C_tang[i] = 0.0;
        R.niter = 0;
        R.norm_res = n0;
        return;
    }
    double acc = 0.0;
    for (int i = 0; i < 6; ++i) {
        R.sigma[i] = trial[i];
        const double ri = trial[i] - sn[i] - Ce[i];
        acc += ri * ri;
    }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) R.C_tang[i * 6 + j] = c_elas_entry(k, i, j);
    R.niter = 1;
    R.norm_res = sqrt(acc);
}
// the same without the tangent (the classify kernel writes C_elas from constants in output order)
DXO_HD void elastic_sigma(const Const& k, const double* sn, const double* Ce, const double* trial, double* sigma, int32_t& niter,
                          double& norm_res) {
    const double n0 = sqrt(dot6(Ce, Ce));
    if (!(n0 / n0 > k.tol)) {
        MC3_UNROLL
        for (int i = 0; i < 6; ++i) sigma[i] = sn[i];
        niter = 0;
        norm_res = n0;
        return;
    }
    double acc = 0.0;
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) {
        sigma[i] = trial[i];
        const double ri = trial[i] - sn[i] - Ce[i];
        acc += ri * ri;
    }
    niter = 1;
    norm_res = sqrt(acc);
}

// State of one plastic point between Newton passes: y = (sig, dl), Y = d y / d deps (7 x 6). As in mc_core.h, where the inputs
// and Y live is a policy: LaneRegs keeps them in the struct (the host build), the kernels of mohr_coulomb3.hip park them in LDS.
struct LaneRegs {
    double deps[6], sn[6];
    double Y[7][6];
    DXO_HD void set_inputs(const double* d, const double* s) {
        for (int i = 0; i < 6; ++i) { deps[i] = d[i]; sn[i] = s[i]; }
    }
    DXO_HD void get_inputs(double* d, double* s) const {
        for (int i = 0; i < 6; ++i) { d[i] = deps[i]; s[i] = sn[i]; }
    }
    DXO_HD void get_col(int m, double* v7) const {
        for (int i = 0; i < 7; ++i) v7[i] = Y[i][m];
    }
    DXO_HD void set_col(int m, const double* v7) {
        for (int i = 0; i < 7; ++i) Y[i][m] = v7[i];
    }
};

template <class Store>
struct LaneT {
    Store st;
    double sig[6], dl;
    double norm0, norm;
    int32_t niter;
};
using Lane = LaneT<LaneRegs>;

template <class Store>
DXO_HD void lane_init(LaneT<Store>& L, const double* deps, const double* sn) {
    L.st.set_inputs(deps, sn);
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) L.sig[i] = sn[i];
    L.dl = 0.0;
    const double zero[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    MC3_UNROLL
    for (int m = 0; m < 6; ++m) L.st.set_col(m, zero);
    L.norm0 = -1.0;  // "not evaluated yet"
    L.norm = 0.0;
    L.niter = 0;
}

// One pass, as mc::lane_pass: surface at the iterate, residual and cond_fun; then the Newton step and the tangent recursion.
// Returns true when the point is finished (converged, NaN, or niter == nitermax).
template <bool SAME, class Store>
DXO_HD bool lane_pass(const Const& k, LaneT<Store>& L) {
    Surf e;
    surf_eval<SAME>(k, L.sig, e);
    double gradg[6], r_sig[6], r_f;
    grad_surface(k, e, 1, gradg);
    {
        double deps[6], sn[6];
        L.st.get_inputs(deps, sn);
        L.norm = residual(k, e, L.sig, L.dl, deps, sn, gradg, r_sig, &r_f);
    }
    if (L.norm0 < 0.0 || L.norm0 != L.norm0) L.norm0 = (L.niter == 0) ? L.norm : L.norm0;
    if (!((L.norm / L.norm0 > k.tol) && (L.niter < k.nitermax))) return true;
    // hess(g) dense, once per pass; M = S + dlambda H_g
    Sym6 H;
    double av[6], bv[6];
    hess_dense(e, 1, H, av, bv);
    Ldl F;
    {
        Sym6 M;
        const double sd = k.inv_E * ((1.0 + k.nu) - k.nu), so = -(k.inv_E * k.nu), ss = k.inv_E * (1.0 + k.nu);
        MC3_UNROLL
        for (int i = 0; i < 6; ++i) {
            MC3_UNROLL
            for (int j = i; j < 6; ++j)
                M.m[sidx(i, j)] = (i == j ? (i < 3 ? sd : ss) : (j < 3 ? so : 0.0)) + L.dl * H.m[sidx(i, j)];
        }
        ldl_factor(M, F);
    }
    double gradf[6];
    if constexpr (SAME) {
        MC3_UNROLL
        for (int i = 0; i < 6; ++i) gradf[i] = gradg[i];
    } else {
        grad_surface(k, e, 0, gradf);
    }
    // Newton step t = J^-1 r
    double rho[6], xh[6], bh[6];
    mc3::S_times(k, r_sig, rho);
    ldl_solve(F, rho, xh);
    ldl_solve(F, gradg, bh);
    const double icb = mc::mc_recip(dot6(gradf, bh));   // the Schur complement's pivot
    const double t_l = (dot6(gradf, xh) - r_f) * icb;
    double t_s[6];
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) t_s[i] = xh[i] - bh[i] * t_l;
    // tangent recursion Y <- J^-1 ([C; 0] + (D J[Y]) t), column by column, in place
    double Ht[6], Hft[6];
    sym_apply(H, t_s, Ht);
    if constexpr (SAME) {
        MC3_UNROLL
        for (int i = 0; i < 6; ++i) Hft[i] = Ht[i];
    } else {
        hess_apply(e, 0, t_s, Hft);
    }
    // T(t_s) = D_t hess(g) dense, once per pass; the columns need dlambda T v + t_l H v = W v, so W takes T's registers and
    // H's are free from here on
    Sym6 W;
    third_dense(e, 1, t_s, av, bv, W);
    MC3_UNROLL
    for (int n = 0; n < 21; ++n) W.m[n] = L.dl * W.m[n] + t_l * H.m[n];
    MC3_UNROLL
    for (int m = 0; m < 6; ++m) {
        double col[7];
        L.st.get_col(m, col);
        const double dlm = col[6];
        double Wv[6], rhs[6], zh[6];
        sym_apply(W, col, Wv);
        MC3_UNROLL
        for (int i = 0; i < 6; ++i) rhs[i] = (i == m ? 1.0 : 0.0) + dlm * Ht[i] + Wv[i];
        const double nu_m = dot6(Hft, col);
        ldl_solve(F, rhs, zh);
        const double mu_m = (dot6(gradf, zh) - nu_m) * icb;
        MC3_UNROLL
        for (int i = 0; i < 6; ++i) col[i] = zh[i] - bh[i] * mu_m;
        col[6] = mu_m;
        L.st.set_col(m, col);
    }
    MC3_UNROLL
    for (int i = 0; i < 6; ++i) L.sig[i] -= t_s[i];
    L.dl -= t_l;
    L.niter += 1;
    return false;
}

DXO_HD void return_map(const Const& k, const double* deps, const double* sn, Result& R) {
    double Ce[6], trial[6];
    mc3::C_times(k, deps, Ce);
    for (int i = 0; i < 6; ++i) trial[i] = sn[i] + Ce[i];
    R.yielding = mc3::f_value(k, trial);
    if (R.yielding <= 0.0) {
        elastic_point(k, sn, Ce, trial, R);
        return;
    }
    Lane L;
    lane_init(L, deps, sn);
    if (k.same_angle) { while (!lane_pass<true>(k, L)) {} }
    else { while (!lane_pass<false>(k, L)) {} }
    for (int i = 0; i < 6; ++i) R.sigma[i] = L.sig[i];
    for (int j = 0; j < 6; ++j) {
        double col[7];
        L.st.get_col(j, col);
        for (int i = 0; i < 6; ++i) R.C_tang[i * 6 + j] = col[i];
    }
    R.niter = L.niter;
    R.norm_res = L.norm;
    R.dlambda = L.dl;
}

}  // namespace mc3
