// Host build of csrc/mc3_core.h — TEST AID ONLY: lets the six-component Mohr-Coulomb lane math be checked against the
// referee on the CPU. Never loaded by the product package.
#include <cstdint>
#include <cmath>
#include <cstring>

#include "mc3_core.h"

struct Prm { double E, nu, c, phi, psi, theta_T, a, tol; int32_t nitermax, pad; };

static mc::Const make(const void* prm) {
    Prm p;
    std::memcpy(&p, prm, sizeof p);
    return mc::make_const(p.E, p.nu, p.c, p.phi, p.psi, p.theta_T, p.a, p.tol, p.nitermax);
}

extern "C" int mc3_core_cpu(const void* prm, int64_t n, const double* deps, const double* sigma_n, double* C_tang,
                            double* sigma, int32_t* niter, double* yielding, double* norm_res, double* dlambda) {
    const mc::Const k = make(prm);
    for (int64_t i = 0; i < n; ++i) {
        mc3::Result R;
        mc3::return_map(k, deps + 6 * i, sigma_n + 6 * i, R);
        std::memcpy(C_tang + 36 * i, R.C_tang, sizeof R.C_tang);
        std::memcpy(sigma + 6 * i, R.sigma, sizeof R.sigma);
        niter[i] = R.niter;
        yielding[i] = R.yielding;
        norm_res[i] = R.norm_res;
        dlambda[i] = R.dlambda;
    }
    return 0;
}

// Dense against structured: out[0..5] = H v dense, [6..11] = H v structured, [12..17] = T(t) v dense, [18..23] = T(t) v
// structured, for the plastic potential g (angle index 1) at the stress `sig`.
extern "C" int mc3_dense_vs_structured(const void* prm, const double* sig, const double* t, const double* v, double* out) {
    const mc::Const k = make(prm);
    mc3::Surf e;
    mc3::surf_eval<false>(k, sig, e);
    mc3::Sym6 H, T;
    double a[6], b[6];
    mc3::hess_dense(e, 1, H, a, b);
    mc3::sym_apply(H, v, out);
    mc3::hess_apply(e, 1, v, out + 6);
    mc3::third_dense(e, 1, t, a, b, T);
    mc3::sym_apply(T, v, out + 12);
    mc3::Third S;
    mc3::third_setup(e, 1, t, S);
    mc3::third_apply(e, 1, S, v, out + 18);
    return 0;
}

#ifdef MC3_STANDALONE_MAIN
// Stand-alone program for a host sanitizer pass over the lane math: a handful of elastic, plastic, zero and hydrostatic points.
#include <cstdio>
int main() {
    Prm p = {6778.0, 0.25, 3.45, 30 * M_PI / 180, 30 * M_PI / 180, 26 * M_PI / 180, 0.26 * 3.45 / std::tan(30 * M_PI / 180), 1e-8, 200, 0};
    const int n = 5;
    const double deps[n][6] = {{1e-6, -2e-6, 1e-6, 1e-6, 2e-6, -1e-6}, {2e-3, -1e-3, 5e-4, 1e-3, -5e-4, 3e-4}, {0, 0, 0, 0, 0, 0},
                               {1e-3, 1e-3, 1e-3, 0, 0, 0}, {-3e-3, 2e-3, 1e-3, 2e-3, 1e-3, -1e-3}};
    const double sn[n][6] = {{-1, -1.2, -0.8, 0.1, 0.05, -0.02}, {-1, -1.2, -0.8, 0.1, 0.05, -0.02}, {0.1, 0.2, 0.1, 0, 0, 0},
                             {1, 1, 1, 0, 0, 0}, {0.1, 0.1, 0.1, 0, 0, 0}};
    double Ct[n][36], s[n][6], y[n], nr[n], dl[n];
    int32_t it[n];
    mc3_core_cpu(&p, n, &deps[0][0], &sn[0][0], &Ct[0][0], &s[0][0], it, y, nr, dl);
    for (int i = 0; i < n; ++i) std::printf("%d niter %d yielding %g sigma0 %g C00 %g\n", i, it[i], y[i], s[i][0], Ct[i][0]);
    return 0;
}
#endif
