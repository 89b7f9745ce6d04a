// lanczos_check.cpp — the Lanczos recurrence of the solvers (openvqe_amd/csrc/sv_lanczos_host.hpp) compiled alone with g++ (ASan + UBSan:
// tests/test_lanczos_host.py) and run on a dense symmetric matrix.  DenseSpace is what RegisterSpace and SectorSpace are on the device:
// vectors are std::vector<double>, the operator is the matrix, an optional 0/1 mask projects the start vector and every update (the
// sector's `reach`), and an optional keep mode retains copies of v_0..v_{m-2} up to a limit and builds the Ritz vector from them in one
// pass (the register's "lanczos_keep_gb").  An apply() can be told to fail, and every call can be logged with its buffers and scalars.
//   usage: lanczos_check <input> <mode> <tol> <max_iter> [<vector output> [<call log>]]
//     input:  int64 n, int64 has_mask, n*n doubles (row-major matrix), n doubles (mask, if has_mask), n doubles (start vector)
//     mode:   two | keep | keep<limit> | fail<k>   (fail<k>: the k-th apply() returns 7)
//     prints: rc, lam, residual, m, an FNV-1a hash over the bytes of alpha and beta, tridiag_lowest on (alpha, beta) once more
//             (eigenvalue and |s|^2 - 1), and the number of vector operations issued after a failed call
//     vector output: the Ritz vector (n doubles), alpha (m), beta (m - 1)
#include "../../openvqe_amd/csrc/sv_lanczos_host.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>

using namespace ovqe;

struct DenseSpace {
    typedef std::vector<double> *Vec;
    int n = 0;
    std::vector<double> mat, mask, start_vec;   // mask empty: none
    std::vector<double> buf[4];                 // v_{j-1}, v_j, w, Ritz vector
    bool keeping = false;
    size_t keep_limit = 0;
    std::deque<std::vector<double>> kept;
    int fail_apply = 0, applies = 0;   // fail_apply = k > 0: the k-th apply() returns 7
    bool failed = false;
    int after_failure = 0;             // vector operations issued after a call has failed
    FILE *log = nullptr;

    std::string name(Vec v) const {
        static const char *names[4] = {"work0", "work1", "work2", "ritz"};
        for (int i = 0; i < 4; ++i)
            if (v == &buf[i]) return names[i];
        for (size_t k = 0; k < kept.size(); ++k)
            if (v == &kept[k]) return "kept" + std::to_string(k);
        return v ? "?" : "null";
    }
    void enter() { if (failed) ++after_failure; }

    Vec work(int i) { return &buf[i]; }
    Vec ritz() { return &buf[3]; }
    int start(Vec v) {
        enter();
        if (log) std::fprintf(log, "start %s\n", name(v).c_str());
        double n2 = 0.0;
        for (int i = 0; i < n; ++i) {
            (*v)[i] = mask.empty() || mask[i] != 0.0 ? start_vec[i] : 0.0;
            n2 += (*v)[i] * (*v)[i];
        }
        for (int i = 0; i < n; ++i) (*v)[i] *= 1.0 / std::sqrt(n2);
        return 0;
    }
    int apply(Vec out, Vec in) {
        enter();
        if (log) std::fprintf(log, "apply %s %s\n", name(out).c_str(), name(in).c_str());
        if (++applies == fail_apply) {
            failed = true;
            return 7;
        }
        for (int i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += mat[(size_t)i * n + k] * (*in)[k];
            (*out)[i] = acc;
        }
        return 0;
    }
    int dot(Vec a, Vec b, double *re) {
        enter();
        if (log) std::fprintf(log, "dot %s %s\n", name(a).c_str(), name(b).c_str());
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += (*a)[i] * (*b)[i];
        *re = acc;
        return 0;
    }
    int update(Vec w, Vec v, Vec vprev, double alpha, double beta, double *norm2) {
        enter();
        if (log) std::fprintf(log, "update %s %s %s %.17g %.17g\n", name(w).c_str(), name(v).c_str(), name(vprev).c_str(), alpha, beta);
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            double x = (*w)[i] - alpha * (*v)[i];
            if (vprev) x -= beta * (*vprev)[i];
            if (!mask.empty() && mask[i] == 0.0) x = 0.0;
            (*w)[i] = x;
            acc += x * x;
        }
        *norm2 = acc;
        return 0;
    }
    int scale(Vec v, double a) {
        enter();
        if (log) std::fprintf(log, "scale %s %.17g\n", name(v).c_str(), a);
        for (int i = 0; i < n; ++i) (*v)[i] *= a;
        return 0;
    }
    int axpy(Vec y, Vec x, double a, bool first) {
        enter();
        if (log) std::fprintf(log, "axpy %s %s %.17g %d\n", name(y).c_str(), name(x).c_str(), a, first ? 1 : 0);
        for (int i = 0; i < n; ++i) (*y)[i] = (first ? 0.0 : (*y)[i]) + a * (*x)[i];
        return 0;
    }
    int keep(Vec vj) {
        enter();
        if (!keeping) return 0;
        if (kept.size() < keep_limit) {
            if (log) std::fprintf(log, "keep %s\n", name(vj).c_str());
            kept.push_back(*vj);
        } else {   // the budget is spent: drop what was kept, pass 2 will run
            if (log) std::fprintf(log, "drop\n");
            kept.clear();
            keeping = false;
        }
        return 0;
    }
    int ritz_from_kept(const std::vector<double> &s, int m, bool *done) {
        enter();
        *done = keeping && (int)kept.size() == m - 1;
        if (!*done) {
            kept.clear();
            keeping = false;
            return 0;
        }
        // v_{m-1} is in the work buffer the rotation left it in: one buffer per step, starting from work1
        Vec ring[3] = {&buf[1], &buf[2], &buf[0]};
        for (int j = 0; j < m; ++j)
            if (int rc = axpy(&buf[3], j < m - 1 ? &kept[j] : ring[(m - 1) % 3], s[j], j == 0)) return rc;
        return 0;
    }
    int release_kept() {   // (runs after a failure too: not counted in after_failure)
        if (log) std::fprintf(log, "release\n");
        kept.clear();
        keeping = false;
        return 0;
    }
};

static bool read_input(const char *path, DenseSpace &V) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    int64_t head[2] = {0, 0};
    bool ok = std::fread(head, sizeof(int64_t), 2, f) == 2 && head[0] >= 1 && head[0] <= 4096;
    if (ok) {
        const size_t n = (size_t)head[0];
        V.n = (int)n;
        V.mat.resize(n * n);
        V.start_vec.resize(n);
        if (head[1]) V.mask.resize(n);
        ok = std::fread(V.mat.data(), sizeof(double), n * n, f) == n * n;
        if (ok && head[1]) ok = std::fread(V.mask.data(), sizeof(double), n, f) == n;
        if (ok) ok = std::fread(V.start_vec.data(), sizeof(double), n, f) == n;
        for (std::vector<double> &b : V.buf) b.assign(n, 0.0);
    }
    std::fclose(f);
    return ok;
}

static uint64_t fnv1a(uint64_t hash, const std::vector<double> &v) {
    const unsigned char *p = (const unsigned char *)v.data();
    for (size_t k = 0; k < v.size() * sizeof(double); ++k) hash = (hash ^ p[k]) * 1099511628211ull;
    return hash;
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: lanczos_check <input> two|keep[<limit>]|fail<k> <tol> <max_iter> [<vector output> [<call log>]]\n");
        return 2;
    }
    DenseSpace V;
    if (!read_input(argv[1], V)) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const std::string mode = argv[2];
    if (mode.compare(0, 4, "keep") == 0) {
        V.keeping = true;
        V.keep_limit = mode.size() > 4 ? (size_t)std::atoi(mode.c_str() + 4) : (size_t)V.n;
    } else if (mode.compare(0, 4, "fail") == 0) {
        V.fail_apply = std::atoi(mode.c_str() + 4);
    } else if (mode != "two") {
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    }
    const double tol = std::atof(argv[3]);
    // the caller caps max_iter at the dimension of the space: the members of the mask, as run_sector_ground_state does
    int dim = V.n;
    if (!V.mask.empty()) {
        dim = 0;
        for (double x : V.mask) dim += x != 0.0;
    }
    const int max_iter = std::min(std::atoi(argv[4]), std::max(dim, 1));
    if (argc > 6 && !(V.log = std::fopen(argv[6], "w"))) return 2;

    LanczosResult res;
    const int rc = lanczos_lowest(V, tol, max_iter, res);
    if (V.log) std::fclose(V.log);

    double tlam = 0.0, snorm2 = 1.0;
    if (!rc) {   // tridiag_lowest alone, on the matrix the recurrence built
        std::vector<double> s;
        tridiag_lowest(res.alpha, res.beta, res.m, &tlam, s);
        snorm2 = 0.0;
        for (double x : s) snorm2 += x * x;
    }
    std::printf("rc=%d lam=%.17g residual=%.17g m=%d hash=%016llx tlam=%.17g snorm2m1=%.3e after_failure=%d\n", rc, res.lam, res.residual,
                res.m, (unsigned long long)fnv1a(fnv1a(1469598103934665603ull, res.alpha), res.beta), tlam, snorm2 - 1.0, V.after_failure);
    if (argc > 5 && !rc) {
        FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 2;
        for (const std::vector<double> *v : {&V.buf[3], &res.alpha, &res.beta})
            if (!v->empty()) std::fwrite(v->data(), sizeof(double), v->size(), f);   // (beta is empty at m = 1)
        std::fclose(f);
    }
    return 0;
}
