// hyper3_core.h — per-point fp64 arithmetic of the 3-D hyperelastic kernels (hyper3.hip): the analytic Isihara model for a 3x3
// deformation gradient, and the wave-level staging that writes a point's 9 stresses and 81 tangent entries in output order.
// W(F) = c1 (I1bar - 3) + c2 (I2bar - 3) + c3 (I1bar - 3)^2 + c4 (J - 1)^2, I1bar = J^(-2/3) I1, I2bar = J^(-4/3) I2, I1 = tr C,
// I2 = (I1^2 - tr C^2) / 2, C = F^T F, J = det F: the full 3-D form of the energy of hyper_core.h (demo_hyperelasticity.py:686-703),
// whose plane-strain statements I1 = tr C_2 + 1, I2 = I1 + J^2 - 1 it gives for F = [[F_2, 0], [0, 1]]. c3 = 0 is the compressible
// Mooney-Rivlin solid, c2 = c3 = 0 the neo-Hookean one.
#pragma once

#include "hyper_core.h"
#include "operand_core.h"

namespace {

constexpr int HYPER3_SYM = 45;   // unique entries of the 9x9 tangent

// entry (I, J), I <= J, of the packed upper triangle, rows in order
__host__ __device__ constexpr int hyper3_tri(int I, int J) { return I * 9 - I * (I - 1) / 2 + (J - I); }
__host__ __device__ constexpr int hyper3_eps(int i, int j, int k) { return (i - j) * (j - k) * (k - i) / 2; }

// P[9] (row-major, F_ia at 3 i + a) and the upper triangle H[45] of dP/dF, a Hessian. W is a function of the generators t = F:F,
// s = C:C and D = det F with
//   grad t = 2 F, grad s = 4 F C =: gs, grad D = cof F =: gD,
//   d2t = 2 d_ij d_ab, d2s = 4 (d_ij C_ab + F_ib F_ja + (F F^T)_ij d_ab), d2D = e_ijk e_abc F_kc,
// and W_ts = W_ss = 0, so
//   P_I  = 2 W_t F_I + W_s gs_I + W_D gD_I
//   H_IJ = 2 W_t d_IJ + W_s d2s + W_D d2D + 4 W_tt F_I F_J + 2 W_tD (F_I gD_J + gD_I F_J) + W_DD gD_I gD_J + W_sD (gs_I gD_J + gD_I gs_J).
// The stress comes first and leaves (hyper3.hip stores it before the tangent is formed); what the tangent needs stays in Isi3Point:
// 27 doubles and 7 coefficients. The C_ab and (F F^T)_ij terms are added in a last sweep that forms each of the twelve sums, adds it
// to its three entries and drops it, so neither matrix is held beside the 45 entries.
// det F <= 0: J^(-2/3) is NaN (UFL's real power), it reaches every first and second derivative of W and so all 90 outputs.
struct Isi3Point {
    double F[9], gs[9], gD[9];
    double Wt2, Ws4, WD, Wtt4, WtD2, WDD, WsD;
};

__device__ __forceinline__ void isihara3_stress(const IsiPrm& prm, const double (&F)[9], Isi3Point& q, double (&P)[9]) {
    double C[3][3];   // F^T F
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) C[a][b] = C[b][a] = F[a] * F[b] + F[3 + a] * F[3 + b] + F[6 + a] * F[6 + b];
    const double t = C[0][0] + C[1][1] + C[2][2];
    const double s = C[0][0] * C[0][0] + C[1][1] * C[1][1] + C[2][2] * C[2][2] +
                     2.0 * (C[0][1] * C[0][1] + C[0][2] * C[0][2] + C[1][2] * C[1][2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            q.F[3 * i + a] = F[3 * i + a];
            q.gs[3 * i + a] = 4.0 * (F[3 * i] * C[0][a] + F[3 * i + 1] * C[1][a] + F[3 * i + 2] * C[2][a]);
            q.gD[3 * i + a] = F[3 * j + b] * F[3 * k + c] - F[3 * j + c] * F[3 * k + b];
        }
    }
    const double D = F[0] * q.gD[0] + F[1] * q.gD[1] + F[2] * q.gD[2];
    const double iD = 1.0 / D;
    const double m = D > 0.0 ? hyper_pow_m23(D) : __builtin_nan(""), nn = m * m;
    const double A = m * t, Bq = 0.5 * nn * (t * t - s);           // I1bar, I2bar
    const double g1 = prm.c1 + 2.0 * prm.c3 * (A - 3.0);
    const double A_D = (-2.0 / 3.0) * A * iD, A_tD = (-2.0 / 3.0) * m * iD, A_DD = (10.0 / 9.0) * A * iD * iD;
    const double B_D = (-4.0 / 3.0) * Bq * iD, B_tD = (-4.0 / 3.0) * nn * t * iD, B_sD = (2.0 / 3.0) * nn * iD,
                 B_DD = (28.0 / 9.0) * Bq * iD * iD;
    const double Ws = -0.5 * prm.c2 * nn;
    q.Wt2 = 2.0 * (g1 * m + prm.c2 * nn * t);
    q.Ws4 = 4.0 * Ws;
    q.WD = g1 * A_D + prm.c2 * B_D + 2.0 * prm.c4 * (D - 1.0);
    q.Wtt4 = 4.0 * (2.0 * prm.c3 * nn + prm.c2 * nn);
    q.WtD2 = 2.0 * (2.0 * prm.c3 * A_D * m + g1 * A_tD + prm.c2 * B_tD);
    q.WsD = prm.c2 * B_sD;
    q.WDD = 2.0 * prm.c3 * A_D * A_D + g1 * A_DD + prm.c2 * B_DD + 2.0 * prm.c4;
#pragma unroll
    for (int I = 0; I < 9; ++I) P[I] = q.Wt2 * F[I] + Ws * q.gs[I] + q.WD * q.gD[I];
}

__device__ __forceinline__ void isihara3_tangent(const Isi3Point& q, double (&H)[HYPER3_SYM]) {
#pragma unroll
    for (int I = 0; I < 9; ++I) {
#pragma unroll
        for (int J = I; J < 9; ++J) {
            const int i = I / 3, a = I % 3, j = J / 3, b = J % 3;
            double h = fma(q.Wtt4, q.F[I] * q.F[J],
                           fma(q.WtD2, fma(q.F[I], q.gD[J], q.gD[I] * q.F[J]),
                               fma(q.WDD, q.gD[I] * q.gD[J],
                                   fma(q.WsD, fma(q.gs[I], q.gD[J], q.gD[I] * q.gs[J]), q.Ws4 * (q.F[3 * i + b] * q.F[3 * j + a])))));
            if (I == J) h += q.Wt2;
            if (i != j && a != b) h = fma(q.WD * (double)(hyper3_eps(i, j, 3 - i - j) * hyper3_eps(a, b, 3 - a - b)), q.F[3 * (3 - i - j) + (3 - a - b)], h);
            H[hyper3_tri(I, J)] = h;
        }
    }
    // d_ij C_ab and (F F^T)_ij d_ab. The empty asm makes the copy of F opaque: the compiler would otherwise recognise the C of the
    // stress in these sums and carry its six values through the 45 entries (the field kernel then needs scratch)
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        f[k] = q.F[k];
        asm volatile("" : "+v"(f[k]));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const double c = q.Ws4 * (f[a] * f[b] + f[3 + a] * f[3 + b] + f[6 + a] * f[6 + b]);                       // 4 W_s C_ab
            const double g = q.Ws4 * (f[3 * a] * f[3 * b] + f[3 * a + 1] * f[3 * b + 1] + f[3 * a + 2] * f[3 * b + 2]);   // 4 W_s (F F^T)_ab
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                H[hyper3_tri(3 * k + a, 3 * k + b)] += c;
                H[hyper3_tri(3 * a + k, 3 * b + k)] += g;
            }
        }
}

// t = H : dF without H, the H_IJ formula above contracted with dF term by term (the array-free action, hyper3_form.h):
//   t_I = 2 W_t dF_I + W_s d2s[dF]_I + W_D d2D[dF]_I + 4 W_tt F_I (F:dF) + 2 W_tD (F_I (gD:dF) + gD_I (F:dF)) + W_DD gD_I (gD:dF)
//         + W_sD (gs_I (gD:dF) + gD_I (gs:dF)),
//   d2s[dF] = 4 (dF C + F dF^T F + F F^T dF) = 4 (dF C + F (N + N^T)), N = dF^T F;   d2D[dF]_ia = e_ijk e_abc dF_jb F_kc,
// the directional derivative of the cofactor. About 150 flops from the point's 27 doubles and 7 coefficients.
// det F <= 0: the coefficients are NaN, and 2 W_t dF_I alone makes every t_I NaN, also where dF = 0.
__device__ __forceinline__ void isihara3_tangent_times(const Isi3Point& q, const double (&dF)[9], double (&t)[9]) {
    const double (&F)[9] = q.F;
    double fd = 0.0, dd = 0.0, sd = 0.0;      // F:dF, gD:dF, gs:dF
#pragma unroll
    for (int I = 0; I < 9; ++I) {
        fd = fma(F[I], dF[I], fd);
        dd = fma(q.gD[I], dF[I], dd);
        sd = fma(q.gs[I], dF[I], sd);
    }
    double C[3][3], S[3][3];      // F^T F; N + N^T
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            C[a][b] = C[b][a] = F[a] * F[b] + F[3 + a] * F[3 + b] + F[6 + a] * F[6 + b];
            S[a][b] = S[b][a] = (dF[a] * F[b] + dF[3 + a] * F[3 + b] + dF[6 + a] * F[6 + b]) +
                                (dF[b] * F[a] + dF[3 + b] * F[3 + a] + dF[6 + b] * F[6 + a]);
        }
    const double cF = fma(q.Wtt4, fd, q.WtD2 * dd);                          // of F_I
    const double cD = fma(q.WtD2, fd, fma(q.WDD, dd, q.WsD * sd));           // of gD_I
    const double cs = q.WsD * dd;                                            // of gs_I
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3, I = 3 * i + a;
            const double d2s = (dF[3 * i] * C[0][a] + dF[3 * i + 1] * C[1][a] + dF[3 * i + 2] * C[2][a]) +
                               (F[3 * i] * S[0][a] + F[3 * i + 1] * S[1][a] + F[3 * i + 2] * S[2][a]);
            const double d2D = (dF[3 * j + b] * F[3 * k + c] - dF[3 * j + c] * F[3 * k + b]) +
                               (F[3 * j + b] * dF[3 * k + c] - F[3 * j + c] * dF[3 * k + b]);
            t[I] = fma(q.Wt2, dF[I], fma(q.Ws4, d2s, fma(q.WD, d2D, fma(cF, F[I], fma(cD, q.gD[I], cs * q.gs[I])))));
        }
    }
}

// ---- the general form: W any function of (t, s, D), given by its nine partials at the point (the network of icnn.hip, whose feature
// K2 is linear in s and whose Hessian couples all three features, so W_ts and W_ss do not vanish):
//   P_I  = 2 W_t F_I + W_s gs_I + W_D gD_I
//   H_IJ = 2 W_t d_IJ + W_s d2s + W_D d2D + 4 W_tt F_I F_J + 2 W_ts (F_I gs_J + gs_I F_J) + 2 W_tD (F_I gD_J + gD_I F_J)
//          + W_ss gs_I gs_J + W_sD (gs_I gD_J + gD_I gs_J) + W_DD gD_I gD_J.
// A stress correction P += h F, H_IJ += h d_IJ (a multiple of the identity) rides in 2 W_t.
struct Hyper3W { double t, s, D, tt, ts, tD, ss, sD, DD; };

// t = F:F, s = C:C, D = det F
__device__ __forceinline__ void hyper3_generators(const double (&F)[9], double& t, double& s, double& D) {
    double C[6];   // 00 01 02 11 12 22
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) C[k++] = F[a] * F[b] + F[3 + a] * F[3 + b] + F[6 + a] * F[6 + b];
    t = C[0] + C[3] + C[5];
    s = C[0] * C[0] + C[3] * C[3] + C[5] * C[5] + 2.0 * (C[1] * C[1] + C[2] * C[2] + C[4] * C[4]);
    D = F[0] * (F[4] * F[8] - F[5] * F[7]) + F[1] * (F[5] * F[6] - F[3] * F[8]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
}

struct Gen3Point {
    double F[9], gs[9], gD[9];
    double Wt2, Ws4, WD, Wtt4, Wts2, WtD2, Wss, WsD, WDD;
};

__device__ __forceinline__ void hyper3_general_stress(const Hyper3W& w, double h, const double (&F)[9], Gen3Point& q, double (&P)[9]) {
    double C[3][3];   // F^T F
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) C[a][b] = C[b][a] = F[a] * F[b] + F[3 + a] * F[3 + b] + F[6 + a] * F[6 + b];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            q.F[3 * i + a] = F[3 * i + a];
            q.gs[3 * i + a] = 4.0 * (F[3 * i] * C[0][a] + F[3 * i + 1] * C[1][a] + F[3 * i + 2] * C[2][a]);
            q.gD[3 * i + a] = F[3 * j + b] * F[3 * k + c] - F[3 * j + c] * F[3 * k + b];
        }
    }
    q.Wt2 = 2.0 * w.t + h;
    q.Ws4 = 4.0 * w.s;
    q.WD = w.D;
    q.Wtt4 = 4.0 * w.tt;
    q.Wts2 = 2.0 * w.ts;
    q.WtD2 = 2.0 * w.tD;
    q.Wss = w.ss;
    q.WsD = w.sD;
    q.WDD = w.DD;
#pragma unroll
    for (int I = 0; I < 9; ++I) P[I] = q.Wt2 * F[I] + w.s * q.gs[I] + q.WD * q.gD[I];
}

// 4 W_s C_ab and 4 W_s (F F^T)_ab, the six unique entries of each (00 01 02 11 12 22): the d_ij C_ab and (F F^T)_ij d_ab terms of d2s
struct Gen3Sums { double c[6], g[6]; };
__host__ __device__ constexpr int hyper3_sym3(int a, int b) { return a <= b ? a * 3 - a * (a - 1) / 2 + (b - a) : hyper3_sym3(b, a); }

__device__ __forceinline__ void hyper3_general_sums(const Gen3Point& q, Gen3Sums& m) {
    const double (&f)[9] = q.F;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            m.c[hyper3_sym3(a, b)] = q.Ws4 * (f[a] * f[b] + f[3 + a] * f[3 + b] + f[6 + a] * f[6 + b]);
            m.g[hyper3_sym3(a, b)] = q.Ws4 * (f[3 * a] * f[3 * b] + f[3 * a + 1] * f[3 * b + 1] + f[3 * a + 2] * f[3 * b + 2]);
        }
}

// entry (I, J), I <= J, of the general tangent
__device__ __forceinline__ double hyper3_general_entry(const Gen3Point& q, const Gen3Sums& m, int I, int J) {
    const int i = I / 3, a = I % 3, j = J / 3, b = J % 3;
    const double FI = q.F[I], FJ = q.F[J], sI = q.gs[I], sJ = q.gs[J], dI = q.gD[I], dJ = q.gD[J];
    double h = fma(q.Wtt4, FI * FJ,
                   fma(q.Wts2, fma(FI, sJ, sI * FJ),
                       fma(q.WtD2, fma(FI, dJ, dI * FJ),
                           fma(q.Wss, sI * sJ,
                               fma(q.WsD, fma(sI, dJ, dI * sJ), fma(q.WDD, dI * dJ, q.Ws4 * (q.F[3 * i + b] * q.F[3 * j + a])))))));
    if (I == J) h += q.Wt2;
    if (i != j && a != b) h = fma(q.WD * (double)(hyper3_eps(i, j, 3 - i - j) * hyper3_eps(a, b, 3 - a - b)), q.F[3 * (3 - i - j) + (3 - a - b)], h);
    if (i == j) h += m.c[hyper3_sym3(a, b)];
    if (a == b) h += m.g[hyper3_sym3(i, j)];
    return h;
}

// the 45 unique entries (for the staged stores of hyper3_store_tangent)
__device__ __forceinline__ void hyper3_general_tangent(const Gen3Point& q, double (&H)[HYPER3_SYM]) {
    Gen3Sums m;
    hyper3_general_sums(q, m);
#pragma unroll
    for (int I = 0; I < 9; ++I)
#pragma unroll
        for (int J = I; J < 9; ++J) H[hyper3_tri(I, J)] = hyper3_general_entry(q, m, I, J);
}

// the same entries, each stored to both of its places in the point's own row dPp[81] the moment it exists: nothing but the point's 27
// doubles, its coefficients and the twelve sums waits in registers
__device__ __forceinline__ void hyper3_general_tangent_rows(const Gen3Point& q, double* __restrict__ dPp) {
    Gen3Sums m;
    hyper3_general_sums(q, m);
#pragma unroll
    for (int I = 0; I < 9; ++I)
#pragma unroll
        for (int J = I; J < 9; ++J) {
            const double h = hyper3_general_entry(q, m, I, J);
            dPp[I * 9 + J] = h;
            if (J != I) dPp[J * 9 + I] = h;
        }
}

// ---- output-ordered stores. A point's tangent is 81 doubles and its stress 9, both odd: a run of points starts 16-byte aligned only
// at an even point and ends on a single double when it holds an odd number of them. The wave stages a run in its LDS buffer X at the
// PARITY of the run's global address (in doubles), so a pair of doubles that is 16-byte aligned in memory is 16-byte aligned in LDS
// too: an unaligned first double, then 16 bytes per lane and 1 KiB of consecutive addresses per store instruction, then a last
// single double.
__device__ __forceinline__ int hyper3_parity(const double* g) { return (int)(((uintptr_t)g >> 3) & 1u); }

template <bool NT>
__device__ __forceinline__ void hyper3_put(double v, double* g) {
    if constexpr (NT) __builtin_nontemporal_store(v, g);
    else *g = v;
}

// X[par .. par + len) -> g[0 .. len), par = hyper3_parity(g)
template <bool NT>
__device__ __forceinline__ void hyper3_store_run(const double* X, double* g, int len, int lane) {
    const int par = hyper3_parity(g);
    if (len <= 0) return;
    if (par && lane == 0) hyper3_put<NT>(X[1], g);
    const int pairs = (len - par) >> 1;
    const dxo_f64x2* X2 = reinterpret_cast<const dxo_f64x2*>(X + 2 * par);
    dxo_f64x2* g2 = reinterpret_cast<dxo_f64x2*>(g + par);
#pragma unroll 4
    for (int idx = lane; idx < pairs; idx += DXO_WAVE) {
        if constexpr (NT) __builtin_nontemporal_store(X2[idx], g2 + idx);
        else g2[idx] = X2[idx];
    }
    if (((len - par) & 1) && lane == 0) hyper3_put<NT>(X[par + len - 1], g + len - 1);
}

// The wave's points (lane = point, `npts` of them, results in registers) through the wave's LDS buffer X of at least pp * 81 + 2
// doubles, pp >= 8: the stresses of all points as one run to P[npts][9]; the tangent to dP[npts][81] in passes of pp points, each a
// run of pp * 81 consecutive doubles, every lane of the pass writing its full rows from the 45 unique entries.
template <bool NT>
__device__ __forceinline__ void hyper3_store_stress(double* X, int lane, int npts, const double (&Pv)[9], double* __restrict__ P) {
    if (lane < npts) {
        double* Xr = X + hyper3_parity(P) + lane * 9;
#pragma unroll
        for (int I = 0; I < 9; ++I) Xr[I] = Pv[I];
    }
    op_fence();
    hyper3_store_run<NT>(X, P, npts * 9, lane);
    op_fence();
}

// the stresses in passes of pp points, for a buffer X smaller than a whole wave's (at least pp * 9 + 2 doubles)
template <bool NT>
__device__ __forceinline__ void hyper3_store_stress_passes(double* X, int pp, int lane, int npts, const double (&Pv)[9],
                                                           double* __restrict__ P) {
    for (int q0 = 0; q0 < npts; q0 += pp) {
        const int nrun = npts - q0 < pp ? npts - q0 : pp;
        double* g = P + (int64_t)q0 * 9;
        const int r = lane - q0;
        if (r >= 0 && r < nrun) {
            double* Xr = X + hyper3_parity(g) + r * 9;
#pragma unroll
            for (int I = 0; I < 9; ++I) Xr[I] = Pv[I];
        }
        op_fence();
        hyper3_store_run<NT>(X, g, nrun * 9, lane);
        op_fence();
    }
}

template <bool NT>
__device__ __forceinline__ void hyper3_store_tangent(double* X, int pp, int lane, int npts, const double (&H)[HYPER3_SYM],
                                                     double* __restrict__ dP) {
    for (int q0 = 0; q0 < npts; q0 += pp) {
        const int nrun = npts - q0 < pp ? npts - q0 : pp;
        double* g = dP + (int64_t)q0 * 81;
        const int r = lane - q0;
        if (r >= 0 && r < nrun) {
            double* Xr = X + hyper3_parity(g) + r * 81;
#pragma unroll
            for (int I = 0; I < 9; ++I)
#pragma unroll
                for (int J = 0; J < 9; ++J) Xr[I * 9 + J] = H[I <= J ? hyper3_tri(I, J) : hyper3_tri(J, I)];
        }
        op_fence();
        hyper3_store_run<NT>(X, g, nrun * 81, lane);
        op_fence();
    }
}

}  // namespace
