// mc3_referee.cpp — TEST AID ONLY: the reference's Mohr-Coulomb return mapping (invariants, Abbo-Sloan K, surface, f, g,
// r, drdy = jacfwd(r), the lax.while_loop Newton, dsigma_ddeps = jacfwd(return_mapping) THROUGH the loop) restated for the
// six-component Mandel vector (xx, yy, zz, sqrt2 xy, sqrt2 xz, sqrt2 yz) with nested dual numbers, in the manner of
// oracle/mc_oracle.cpp for plane strain. The only change against the plane-strain statement is the tensor algebra: dev, tr
// and C_elas on six components and J3 = det s with all three shears. Instantiated for double (the reference's arithmetic)
// and long double (the accuracy referee).
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace {

template <int N, class R>
struct DualN {
    R v;
    R d[N];
    DualN() : v(0.0) { for (int i = 0; i < N; ++i) d[i] = 0.0; }
    DualN(double c) : v(c) { for (int i = 0; i < N; ++i) d[i] = 0.0; }  // NOLINT
};
template <class T>
struct Dual {
    T v, d;
    Dual() : v(0.0), d(0.0) {}
    Dual(double c) : v(c), d(0.0) {}  // NOLINT
    Dual(const T& v_, const T& d_) : v(v_), d(d_) {}
};

template <int N, class R> inline double primal(const DualN<N, R>& x) { return (double)x.v; }
template <class T> inline double primal(const Dual<T>& x) { return primal(x.v); }

template <int N, class R> inline DualN<N, R> operator+(const DualN<N, R>& a, const DualN<N, R>& b) { DualN<N, R> r; r.v = a.v + b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
template <int N, class R> inline DualN<N, R> operator-(const DualN<N, R>& a, const DualN<N, R>& b) { DualN<N, R> r; r.v = a.v - b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
template <int N, class R> inline DualN<N, R> operator-(const DualN<N, R>& a) { DualN<N, R> r; r.v = -a.v; for (int i = 0; i < N; ++i) r.d[i] = -a.d[i]; return r; }
template <int N, class R> inline DualN<N, R> operator*(const DualN<N, R>& a, const DualN<N, R>& b) { DualN<N, R> r; r.v = a.v * b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
template <int N, class R> inline DualN<N, R> operator/(const DualN<N, R>& a, const DualN<N, R>& b) { DualN<N, R> r; r.v = a.v / b.v; for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) / b.v; return r; }
template <int N, class R> inline DualN<N, R> sqrt(const DualN<N, R>& a) { DualN<N, R> r; r.v = std::sqrt(a.v); for (int i = 0; i < N; ++i) r.d[i] = a.d[i] / (R(2.0) * r.v); return r; }
template <int N, class R> inline DualN<N, R> asin(const DualN<N, R>& a) { DualN<N, R> r; r.v = std::asin(a.v); const R g = R(1.0) / std::sqrt(R(1.0) - a.v * a.v); for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * g; return r; }
template <int N, class R> inline DualN<N, R> sin(const DualN<N, R>& a) { DualN<N, R> r; r.v = std::sin(a.v); const R g = std::cos(a.v); for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * g; return r; }
template <int N, class R> inline DualN<N, R> cos(const DualN<N, R>& a) { DualN<N, R> r; r.v = std::cos(a.v); const R g = -std::sin(a.v); for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * g; return r; }

template <class T> inline Dual<T> operator+(const Dual<T>& a, const Dual<T>& b) { return Dual<T>(a.v + b.v, a.d + b.d); }
template <class T> inline Dual<T> operator-(const Dual<T>& a, const Dual<T>& b) { return Dual<T>(a.v - b.v, a.d - b.d); }
template <class T> inline Dual<T> operator-(const Dual<T>& a) { return Dual<T>(-a.v, -a.d); }
template <class T> inline Dual<T> operator*(const Dual<T>& a, const Dual<T>& b) { return Dual<T>(a.v * b.v, a.d * b.v + a.v * b.d); }
template <class T> inline Dual<T> operator/(const Dual<T>& a, const Dual<T>& b) { T q = a.v / b.v; return Dual<T>(q, (a.d - q * b.d) / b.v); }
template <class T> inline Dual<T> sqrt(const Dual<T>& a) { T s = sqrt(a.v); return Dual<T>(s, a.d / (T(2.0) * s)); }
template <class T> inline Dual<T> asin(const Dual<T>& a) { return Dual<T>(asin(a.v), a.d / sqrt(T(1.0) - a.v * a.v)); }
template <class T> inline Dual<T> sin(const Dual<T>& a) { return Dual<T>(sin(a.v), a.d * cos(a.v)); }
template <class T> inline Dual<T> cos(const Dual<T>& a) { return Dual<T>(cos(a.v), -(a.d * sin(a.v))); }

#define MC3_MIXED(OP)                                                                                                        \
    template <int N, class R> inline DualN<N, R> operator OP(const DualN<N, R>& a, double b) { return a OP DualN<N, R>(b); } \
    template <int N, class R> inline DualN<N, R> operator OP(double a, const DualN<N, R>& b) { return DualN<N, R>(a) OP b; } \
    template <class T> inline Dual<T> operator OP(const Dual<T>& a, double b) { return a OP Dual<T>(b); }                    \
    template <class T> inline Dual<T> operator OP(double a, const Dual<T>& b) { return Dual<T>(a) OP b; }
MC3_MIXED(+)
MC3_MIXED(-)
MC3_MIXED(*)
MC3_MIXED(/)
#undef MC3_MIXED

template <class T> inline T clip(const T& x, double lo, double hi) {   // jnp.clip: no tangent outside
    const double p = primal(x);
    if (p < lo) return T(lo);
    if (p > hi) return T(hi);
    return x;
}

struct Params { double E, nu, c, phi, psi, theta_T, a, tol; int32_t nitermax, pad; };

struct Model {
    Params p;
    double lmbda, mu, coeff3;
    explicit Model(const Params& q) : p(q) {
        lmbda = p.E * p.nu / ((1.0 + p.nu) * (1.0 - 2.0 * p.nu));
        mu = p.E / (2.0 * (1.0 + p.nu));
        coeff3 = 18.0 * std::cos(3.0 * p.theta_T) * std::cos(3.0 * p.theta_T) * std::cos(3.0 * p.theta_T);
    }
    // det of the symmetric 3x3 tensor whose Mandel vector is s
    template <class T> T J3(const T* s) const {
        return s[0] * s[1] * s[2] + s[3] * s[4] * s[5] / std::sqrt(2.0) - 0.5 * (s[0] * s[5] * s[5] + s[1] * s[4] * s[4] + s[2] * s[3] * s[3]);
    }
    template <class T> T J2(const T* s) const {
        T acc = s[0] * s[0];
        for (int i = 1; i < 6; ++i) acc = acc + s[i] * s[i];
        return 0.5 * acc;
    }
    template <class T> T theta(const T* s) const {
        T J2_ = J2(s);
        T arg = -(3.0 * std::sqrt(3.0) * J3(s)) / (2.0 * sqrt(J2_ * J2_ * J2_));
        arg = clip(arg, -1.0, 1.0);
        return (1.0 / 3.0) * asin(arg);
    }
    static int sign(double x) { return x < 0.0 ? -1 : 1; }
    double coeff1(double angle) const { return std::cos(p.theta_T) - (1.0 / std::sqrt(3.0)) * std::sin(angle) * std::sin(p.theta_T); }
    double coeff2(double th, double angle) const { return sign(th) * std::sin(p.theta_T) + (1.0 / std::sqrt(3.0)) * std::sin(angle) * std::cos(p.theta_T); }
    double Cc(double th, double angle) const {
        return (-std::cos(3.0 * p.theta_T) * coeff1(angle) - 3.0 * sign(th) * std::sin(3.0 * p.theta_T) * coeff2(th, angle)) / coeff3;
    }
    double Bc(double th, double angle) const {
        return (sign(th) * std::sin(6.0 * p.theta_T) * coeff1(angle) - 6.0 * std::cos(6.0 * p.theta_T) * coeff2(th, angle)) / coeff3;
    }
    double Ac(double th, double angle) const {
        return -(1.0 / std::sqrt(3.0)) * std::sin(angle) * sign(th) * std::sin(p.theta_T) - Bc(th, angle) * sign(th) * std::sin(3 * p.theta_T) -
               Cc(th, angle) * std::sin(3.0 * p.theta_T) * std::sin(3.0 * p.theta_T) + std::cos(p.theta_T);
    }
    template <class T> T K(const T& th, double angle) const {
        const double thp = primal(th);
        if (std::fabs(thp) > p.theta_T) {
            T s3 = sin(3.0 * th);
            return Ac(thp, angle) + Bc(thp, angle) * s3 + Cc(thp, angle) * s3 * s3;
        }
        return cos(th) - (1.0 / std::sqrt(3.0)) * std::sin(angle) * sin(th);
    }
    double a_g(double angle) const { return p.a * std::tan(p.phi) / std::tan(angle); }
    template <class T> T surface(const T* sig, double angle) const {
        T I1 = sig[0] + sig[1] + sig[2];
        T s[6];
        for (int i = 0; i < 3; ++i) s[i] = sig[i] - I1 / 3.0;
        for (int i = 3; i < 6; ++i) s[i] = sig[i];
        T th = theta(s);
        T Kt = K(th, angle);
        return (I1 / 3.0 * std::sin(angle)) + sqrt(J2(s) * Kt * Kt + a_g(angle) * a_g(angle) * std::sin(angle) * std::sin(angle)) -
               p.c * std::cos(angle);
    }
    template <class T> T f(const T* sig) const { return surface(sig, p.phi); }
    template <class T> T g(const T* sig) const { return surface(sig, p.psi); }
    template <class T> void dgdsigma(const T* sig, T* out) const {   // jacfwd(g)
        for (int i = 0; i < 6; ++i) {
            Dual<T> x[6];
            for (int j = 0; j < 6; ++j) x[j] = Dual<T>(sig[j], T(j == i ? 1.0 : 0.0));
            out[i] = g(x).d;
        }
    }
    template <class T> void C_times(const T* x, T* out) const {
        T t = lmbda * (x[0] + x[1] + x[2]);
        for (int i = 0; i < 3; ++i) out[i] = t + 2.0 * mu * x[i];
        for (int i = 3; i < 6; ++i) out[i] = 2.0 * mu * x[i];
    }
    // r(y, deps, sigma_n); `elastic` is the sign of f at the trial stress, a function of the primal inputs alone
    template <class T> void r(bool elastic, const T* y, const T* deps, const T* sn, T* res) const {
        const T& dlambda = y[6];
        T depsp[6];
        if (elastic) {
            for (int i = 0; i < 6; ++i) depsp[i] = T(0.0);
        } else {
            T gg[6];
            dgdsigma(y, gg);
            for (int i = 0; i < 6; ++i) depsp[i] = dlambda * gg[i];
        }
        T diff[6], Cd[6];
        for (int i = 0; i < 6; ++i) diff[i] = deps[i] - depsp[i];
        C_times(diff, Cd);
        for (int i = 0; i < 6; ++i) res[i] = y[i] - sn[i] - Cd[i];
        res[6] = elastic ? dlambda : f(y);
    }
    template <class T> void drdy(bool elastic, const T* y, const T* deps, const T* sn, T (*J)[7]) const {   // jacfwd(r)
        for (int j = 0; j < 7; ++j) {
            Dual<T> yy[7], dd[6], ss[6], rr[7];
            for (int i = 0; i < 7; ++i) yy[i] = Dual<T>(y[i], T(i == j ? 1.0 : 0.0));
            for (int i = 0; i < 6; ++i) {
                dd[i] = Dual<T>(deps[i], T(0.0));
                ss[i] = Dual<T>(sn[i], T(0.0));
            }
            r(elastic, yy, dd, ss, rr);
            for (int i = 0; i < 7; ++i) J[i][j] = rr[i].d;
        }
    }
};

template <class T> T norm7(const T* r) {
    T acc = r[0] * r[0];
    for (int i = 1; i < 7; ++i) acc = acc + r[i] * r[i];
    return sqrt(acc);
}

// jnp.linalg.solve: LU with partial pivoting by primal magnitude, carried out on T
template <class T> void solve7(T (*A)[7], T* b, T* x) {
    int perm[7] = {0, 1, 2, 3, 4, 5, 6};
    for (int k = 0; k < 7; ++k) {
        int piv = k;
        double best = std::fabs(primal(A[perm[k]][k]));
        for (int i = k + 1; i < 7; ++i) {
            const double v = std::fabs(primal(A[perm[i]][k]));
            if (v > best) { best = v; piv = i; }
        }
        const int tmp = perm[k]; perm[k] = perm[piv]; perm[piv] = tmp;
        const int pk = perm[k];
        for (int i = k + 1; i < 7; ++i) {
            const int pi = perm[i];
            T m = A[pi][k] / A[pk][k];
            for (int j = k + 1; j < 7; ++j) A[pi][j] = A[pi][j] - m * A[pk][j];
            b[pi] = b[pi] - m * b[pk];
        }
    }
    for (int k = 6; k >= 0; --k) {
        const int pk = perm[k];
        T acc = b[pk];
        for (int j = k + 1; j < 7; ++j) acc = acc - A[pk][j] * x[j];
        x[k] = acc / A[pk][k];
    }
}

template <class R>
void run(const void* prm, int64_t n, const double* deps, const double* sigma_n, double* C_tang, double* sigma, int32_t* niter,
         double* yielding, double* norm_res, double* dlambda, int nthreads) {
    Params p;
    std::memcpy(&p, prm, sizeof p);
    const Model M(p);
    typedef DualN<6, R> S;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(nthreads > 1 ? nthreads : 1)
#endif
    for (int64_t i = 0; i < n; ++i) {
        S e[6], s0[6], y[7], res[7];
        for (int k = 0; k < 6; ++k) {
            e[k] = S(deps[i * 6 + k]);
            e[k].d[k] = R(1.0);   // jacfwd seeds
            s0[k] = S(sigma_n[i * 6 + k]);
        }
        S Ce[6], trial[6];
        M.C_times(e, Ce);
        for (int k = 0; k < 6; ++k) trial[k] = s0[k] + Ce[k];
        const double yl = primal(M.f(trial));
        const bool elastic = yl <= 0.0;
        int it = 0;
        for (int k = 0; k < 6; ++k) y[k] = s0[k];
        y[6] = S(0.0);
        M.r(elastic, y, e, s0, res);
        S nr = norm7(res);
        const R nr0 = nr.v;
        while ((nr.v / nr0 > (R)p.tol) && (it < p.nitermax)) {
            S J[7][7], rhs[7], step[7];
            M.drdy(elastic, y, e, s0, J);
            for (int k = 0; k < 7; ++k) rhs[k] = -res[k];
            solve7(J, rhs, step);
            for (int k = 0; k < 7; ++k) y[k] = y[k] + step[k];
            M.r(elastic, y, e, s0, res);
            nr = norm7(res);
            it += 1;
        }
        for (int a = 0; a < 6; ++a) {
            sigma[i * 6 + a] = (double)y[a].v;
            if (C_tang)
                for (int b = 0; b < 6; ++b) C_tang[i * 36 + a * 6 + b] = (double)y[a].d[b];
        }
        if (niter) niter[i] = it;
        if (yielding) yielding[i] = yl;
        if (norm_res) norm_res[i] = (double)nr.v;
        if (dlambda) dlambda[i] = (double)y[6].v;
    }
}

}  // namespace

extern "C" {
int mc3_referee(const void* prm, int64_t n, const double* deps, const double* sigma_n, double* C_tang, double* sigma, int32_t* niter,
                double* yielding, double* norm_res, double* dlambda, int nthreads) {
    run<double>(prm, n, deps, sigma_n, C_tang, sigma, niter, yielding, norm_res, dlambda, nthreads);
    return 0;
}
int mc3_referee_ld(const void* prm, int64_t n, const double* deps, const double* sigma_n, double* C_tang, double* sigma, int32_t* niter,
                   double* yielding, double* norm_res, double* dlambda, int nthreads) {
    run<long double>(prm, n, deps, sigma_n, C_tang, sigma, niter, yielding, norm_res, dlambda, nthreads);
    return 0;
}
}
