// sv_lanczos_host.hpp — the one Lanczos recurrence of the solvers: lowest eigenpair of a Hermitian operator by two-pass Lanczos without
// reorthogonalisation, and the lowest eigenpair of the tridiagonal matrix it builds.  Host-only: no HIP, no handle types — g++ compiles
// it alone (tests/cpu/lanczos_check.cpp runs it on dense matrices under ASan + UBSan).  The recurrence knows vectors only through a
// Space: RegisterSpace (abi_solvers.inc: ovqe_ground_state, amp_t buffers of the whole register) and SectorSpace (sector_host.inc:
// ovqe_sector_ground_state, doubles on the compact support, projected on the block of H reached from the reference determinant).
// ShardedStatevector.ground_state (openvqe_amd/distributed.py) restates the same algorithm in Python over the shards of a register.
//
// A Space provides
//   typedef ... Vec;                       handle of a vector (a pointer type: Vec() means "no vector")
//   Vec work(int i), i = 0, 1, 2;          the three work vectors v_{j-1}, v_j, w;     Vec ritz();   where the eigenvector is built
//   int start(Vec v);                      v = the space's seeded start vector, normalised
//   int apply(Vec out, Vec in);            out = H in
//   int dot(Vec a, Vec b, double *re);     *re = Re <a|b>
//   int update(Vec w, Vec v, Vec vprev, double alpha, double beta, double *norm2);  w -= alpha v + beta vprev;  *norm2 = |w|^2
//   int scale(Vec v, double a);            v *= a
//   int axpy(Vec y, Vec x, double a, bool first);   y = (first ? 0 : y) + a x
// and the three calls of the one-pass form (LanczosTwoPass supplies the "keeps nothing" versions)
//   int keep(Vec vj);                      after step j of pass 1: the space may retain a copy of v_j
//   int ritz_from_kept(s, m, &done);       after pass 1: a space that holds v_0..v_{m-2} (v_{m-1} is still in its work buffer) builds
//                                          ritz() = sum_j s[j] v_j and sets done; otherwise pass 2 repeats the recurrence for it
//   int release_kept();                    the Ritz vector is complete (or the solve failed): wait for it, free what was kept
// Every call returns 0 or a code of the space's own; a non-zero code ends the solve and is returned unchanged.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace ovqe {

// lowest eigenpair of the symmetric tridiagonal matrix (a[0..m), b[0..m-1)): bisection on the Sturm count, then
// inverse iteration with a shift just below the eigenvalue (T - mu is positive definite: LDL^T without pivoting)
inline void tridiag_lowest(const std::vector<double> &a, const std::vector<double> &b, int m, double *lam, std::vector<double> &s) {
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < m; ++i) {
        const double r = (i > 0 ? std::fabs(b[i - 1]) : 0.0) + (i < m - 1 ? std::fabs(b[i]) : 0.0);
        lo = std::min(lo, a[i] - r);
        hi = std::max(hi, a[i] + r);
    }
    const double scale = std::max({std::fabs(lo), std::fabs(hi), 1e-300});
    auto below = [&](double x) {  // number of eigenvalues < x
        int c = 0;
        double d = 1.0;
        for (int i = 0; i < m; ++i) {
            d = a[i] - x - (i > 0 ? b[i - 1] * b[i - 1] / d : 0.0);
            if (std::fabs(d) < 1e-300) d = -1e-300;
            if (d < 0.0) ++c;
        }
        return c;
    };
    for (int it = 0; it < 300 && hi - lo > 4e-16 * scale; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (below(mid) >= 1) hi = mid; else lo = mid;
    }
    *lam = 0.5 * (lo + hi);
    const double mu = *lam - 1e-9 * scale;
    std::vector<double> d(m), l(std::max(m - 1, 0));
    d[0] = a[0] - mu;
    for (int i = 0; i + 1 < m; ++i) {
        l[i] = b[i] / d[i];
        d[i + 1] = a[i + 1] - mu - l[i] * b[i];
    }
    s.assign(m, 1.0 / std::sqrt((double)m));
    for (int it = 0; it < 6; ++it) {
        for (int i = 1; i < m; ++i) s[i] -= l[i - 1] * s[i - 1];
        for (int i = 0; i < m; ++i) s[i] /= d[i];
        for (int i = m - 2; i >= 0; --i) s[i] -= l[i] * s[i + 1];
        double nrm = 0.0;
        for (int i = 0; i < m; ++i) nrm += s[i] * s[i];
        nrm = 1.0 / std::sqrt(nrm);
        for (int i = 0; i < m; ++i) s[i] *= nrm;
    }
}

struct LanczosResult {
    double lam = 0.0;       // Rayleigh quotient of the normalised Ritz vector
    double residual = 0.0;  // |H y - lam y|
    int m = 0;              // steps taken = size of the tridiagonal matrix
    std::vector<double> alpha, beta;  // its diagonal (m) and off-diagonal (m - 1)
};

// a space that retains no Lanczos vector: pass 2 always runs
struct LanczosTwoPass {
    template <class Vec> int keep(Vec) { return 0; }
    int ritz_from_kept(const std::vector<double> &, int, bool *done) { *done = false; return 0; }
    int release_kept() { return 0; }
};

// Lowest eigenpair of the space's operator: V.ritz() holds the normalised eigenvector on return.  max_iter is at most the dimension of
// the space (the caller caps it); tol bounds the Ritz estimate |beta_m s_m| relative to max(1, |lambda|).
template <class Space>
int lanczos_lowest(Space &V, double tol, int max_iter, LanczosResult &out) {
    typedef typename Space::Vec Vec;
    out = LanczosResult();
    std::vector<double> &alpha = out.alpha, &beta = out.beta;
    std::vector<double> s;
    double lam = 0.0;
    int m = 0;
    auto recurrence = [&](bool accumulate) -> int {
        Vec A = V.work(0), B = V.work(1), C = V.work(2);  // v_{j-1}, v_j, w
        int r = V.start(B);
        if (r) return r;
        if (accumulate && (r = V.axpy(V.ritz(), B, s[0], true))) return r;
        const int steps = accumulate ? m - 1 : max_iter;
        for (int j = 0; j < steps; ++j) {
            if ((r = V.apply(C, B))) return r;
            double bj;
            if (accumulate) {
                if ((r = V.update(C, B, j ? A : Vec(), alpha[j], j ? beta[j - 1] : 0.0, &bj))) return r;
                bj = beta[j];
            } else {
                double a;
                if ((r = V.dot(B, C, &a))) return r;
                alpha.push_back(a);
                if ((r = V.update(C, B, j ? A : Vec(), a, j ? beta[j - 1] : 0.0, &bj))) return r;
                bj = std::sqrt(bj);
                m = j + 1;
                const bool last = j + 1 == steps || bj < 1e-13 * std::max(1.0, std::fabs(a));
                if (last || (j >= 4 && j % 5 == 4)) {
                    tridiag_lowest(alpha, beta, m, &lam, s);
                    if (last || std::fabs(bj * s[m - 1]) < tol * std::max(1.0, std::fabs(lam))) return 0;
                }
                beta.push_back(bj);
            }
            if ((r = V.scale(C, 1.0 / bj))) return r;
            if (!accumulate && (r = V.keep(B))) return r;
            Vec t = A;
            A = B;
            B = C;
            C = t;
            if (accumulate && (r = V.axpy(V.ritz(), B, s[j + 1], false))) return r;
        }
        return 0;
    };
    int rc = recurrence(false);  // pass 1: the tridiagonal matrix
    bool done = false;
    if (!rc) rc = V.ritz_from_kept(s, m, &done);
    if (!rc && !done) rc = recurrence(true);  // pass 2: the Ritz vector, same recurrence
    const int released = V.release_kept();
    if (!rc) rc = released;
    if (rc) return rc;
    // normalise, Rayleigh quotient and true residual |H y - lambda y|
    const Vec y = V.ritz(), w = V.work(2);
    double n2 = 0.0;
    if ((rc = V.dot(y, y, &n2))) return rc;
    if ((rc = V.scale(y, 1.0 / std::sqrt(n2)))) return rc;
    if ((rc = V.apply(w, y))) return rc;
    if ((rc = V.dot(y, w, &lam))) return rc;
    if ((rc = V.update(w, y, Vec(), lam, 0.0, &n2))) return rc;
    out.residual = std::sqrt(n2);
    out.lam = lam;
    out.m = m;
    return 0;
}

}  // namespace ovqe
