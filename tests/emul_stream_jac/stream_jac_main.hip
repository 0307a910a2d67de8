// TEST-ONLY stand-alone program (its own main, no Python, nothing preloaded): the x86 build of
// the streamed-row solver's contact-point Jacobian copies on shapes of its own making, for a
// run under the host address and undefined-behaviour sanitizers
// (tests/emul_stream_jac/Makefile, tests/test_stream_jacobian.py).  The Jacobian phase indexes
// the rows at run time like the solve: the row state is a heap array of exactly the kernel's
// LDS size, the row pool exactly the shapes' rows.  Row totals 129, 192, 193, 1,023 and 1,024
// for (N, NSOC) = (4, 0) -- a last slot of one row, full slots, one row over, one short of the
// cap, the cap -- and one pair of each other streamed (N, NSOC), with the FD gradient (shared
// z aggregates) and without a gradient (the phase forms them itself).  Exit status: 0 if every
// pair converged to a finite Jacobian, 1 otherwise.
#include <cmath>
#include <cstdio>
#include <vector>

#include "emul_stream_jac.hpp"

namespace {
// fixed-seed generator (splitmix64), uniform and normal deviates
struct Rng {
    unsigned long long s = 0x9e3779b97f4a7c15ull;
    unsigned long long next() {
        unsigned long long z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 11) * (1.0 / 9007199254740992.0)); }
    double normal() {
        const double u = uni(1e-12, 1.0), v = uni(0.0, 1.0);
        return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
    }
};

struct Shapes {
    std::vector<std::vector<double>> A, b;   // storage the descriptors point into
    std::vector<dcol_shape_desc> d;
    int add(int type, int nh, double R, double L, double H, double beta) {
        dcol_shape_desc s{};
        s.type = type;
        s.nh = nh;
        s.R = R;
        s.L = L;
        s.H = H;
        s.beta = beta;
        for (int k = 0; k < 9; ++k) s.Q_offset[k] = (k % 4 == 0) ? 1.0 : 0.0;
        d.push_back(s);
        return (int)d.size() - 1;
    }
    // bounded random polytope: the 6 box normals plus k - 6 random unit normals, offsets U(0.4, 1.3)
    int polytope(Rng& g, int k) {
        std::vector<double> a(3 * k, 0.0), o(k);
        for (int j = 0; j < 6; ++j) a[3 * j + j % 3] = j < 3 ? 1.0 : -1.0;
        for (int j = 6; j < k; ++j) {
            double v[3] = {g.normal(), g.normal(), g.normal()};
            const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int c = 0; c < 3; ++c) a[3 * j + c] = v[c] / n;
        }
        for (int j = 0; j < k; ++j) o[j] = g.uni(0.4, 1.3);
        A.push_back(a);
        b.push_back(o);
        return add(DCOL_POLYTOPE, k, 0, 0, 0, 0);
    }
    int polygon(int k, double r, double R) {
        std::vector<double> a(2 * k), o(k, r);
        for (int j = 0; j < k; ++j) {
            a[2 * j] = std::cos(6.283185307179586 * j / k);
            a[2 * j + 1] = std::sin(6.283185307179586 * j / k);
        }
        A.push_back(a);
        b.push_back(o);
        return add(DCOL_POLYGON, k, R, 0, 0, 0);
    }
    // the descriptors' pointers, once every shape is made (the storage vectors no longer grow)
    void bind() {
        for (size_t i = 0, k = 0; i < d.size(); ++i)
            if (d[i].nh) {
                d[i].A = A[k].data();
                d[i].b = b[k].data();
                ++k;
            }
    }
};
}  // namespace

int main() {
    using namespace dcol;
    using namespace dcol_host;
    Rng g;
    Shapes S;
    const int box = S.polytope(g, 6), sph = S.add(DCOL_SPHERE, 0, 0.5, 0, 0, 0), cone = S.add(DCOL_CONE, 0, 0, 0, 1.2, 0.4),
              cap = S.add(DCOL_CAPSULE, 0, 0.3, 1.0, 0, 0);
    const int p123 = S.polytope(g, 123), p127 = S.polytope(g, 127), p186 = S.polytope(g, 186), p187 = S.polytope(g, 187),
              p192 = S.polytope(g, 192), p511 = S.polytope(g, 511), p512 = S.polytope(g, 512), p512b = S.polytope(g, 512),
              p723 = S.polytope(g, 723);
    const int g300 = S.polygon(300, 0.6, 0.2), g1023 = S.polygon(1023, 0.6, 0.2);
    S.bind();
    const int pairs[][2] = {{p123, box}, {p186, box}, {p187, box}, {p511, p512}, {p512, p512b},   // (4, 0)
                            {p192, sph},                                                       // (4, 1)
                            {cap, p127},                                                       // (5, 1)
                            {g300, p723},                                                      // (6, 1)
                            {g1023, cone}};                                                    // (6, 2)
    const int B = (int)(sizeof(pairs) / sizeof(pairs[0]));
    std::vector<DevShape> sh(S.d.size());
    std::vector<DevRow> rows;
    init_row_pool(rows);
    for (size_t i = 0; i < S.d.size(); ++i)
        if (digest_shape(S.d[i], (int32_t)i, sh[i], rows)) {
            std::fprintf(stderr, "digest: %s\n", last_error().c_str());
            return 1;
        }
    rows.shrink_to_fit();
    std::vector<int32_t> s1(B), s2(B), iters(B), status(B);
    std::vector<double> p1(6 * B), p2(6 * B), alpha(B), contact(3 * B), grad(12 * B), jac(48 * B);
    for (int i = 0; i < B; ++i) {
        s1[i] = pairs[i][0];
        s2[i] = pairs[i][1];
        for (int q = 0; q < 6; ++q) {
            p1[6 * i + q] = q < 3 ? g.uni(-3, 3) : g.uni(-1, 1);
            p2[6 * i + q] = q < 3 ? g.uni(-3, 3) : g.uni(-1, 1);
        }
    }
    int bad = 0;
    for (const int mode : {(int)DCOL_GRAD_FD, 0}) {
        const int rc = emul_stream_jac::solve_batch(sh, rows, B, s1.data(), s2.data(), p1.data(), p2.data(), 1e-6, 50,
                                                    mode | DCOL_CONTACT | DCOL_JACOBIAN, alpha.data(), contact.data(),
                                                    grad.data(), jac.data(), iters.data(), status.data());
        if (rc) {
            std::fprintf(stderr, "solve: %s\n", last_error().c_str());
            return 1;
        }
        for (int i = 0; i < B; ++i) {
            bool fin = std::isfinite(alpha[i]);
            double jmax = 0.0;
            for (int q = 0; q < 48; ++q) {
                fin = fin && std::isfinite(jac[48 * i + q]);
                jmax = std::fmax(jmax, std::fabs(jac[48 * i + q]));
            }
            const PairClass c = classify(sh[s1[i]], sh[s2[i]]);
            std::printf("mode %2d pair %2d (N, NSOC) (%d, %d) rows %4d status %d iters %2d alpha %.12g max|J| %.6g%s\n", mode, i,
                        c.N, c.nsoc, c.o, status[i], iters[i], alpha[i], jmax, fin ? "" : "  NON-FINITE");
            bad += !fin || status[i] != DCOL_OK;
        }
    }
    return bad ? 1 : 0;
}
