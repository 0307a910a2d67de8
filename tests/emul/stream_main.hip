// TEST-ONLY stand-alone programs (their own main, no Python, nothing preloaded): the x86 build of
// the streamed-row solver on shapes of its own making, for a run under the host address and
// undefined-behaviour sanitizers (tests/emul/Makefile).  The run-time row indexing is where the
// streamed kernel could step out of bounds: the row state is a heap array of exactly the
// kernel's LDS size, the row pool exactly the shapes' rows.  Row totals 129, 192, 193, 1,023
// and 1,024 -- a last slot of one row, full slots, one row over, one short of the cap, the cap.
//   stream_asan (-DEMUL_RUN_JAC=0; tests/test_stream_rows.py): the solve, over every streamed
//     (N, NSOC), in the three gradient modes.
//   stream_jac_asan (-DEMUL_RUN_JAC=1; tests/test_stream_jacobian.py): the contact-point Jacobian
//     copies, whose Jacobian phase indexes the rows at run time like the solve -- those row
//     totals for (N, NSOC) = (4, 0) and one pair of each other streamed (N, NSOC), with the FD
//     gradient (shared z aggregates) and without a gradient (the phase forms them itself).
// Exit status: 0 if every pair converged to finite values, 1 otherwise.
#include <cmath>
#include <cstdio>
#include <vector>

#include "emul_batch.hpp"

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
    using namespace emul;
    Rng g;
    Shapes S;
    const int box = S.polytope(g, 6), sph = S.add(DCOL_SPHERE, 0, 0.5, 0, 0, 0), cone = S.add(DCOL_CONE, 0, 0, 0, 1.2, 0.4),
              cap = S.add(DCOL_CAPSULE, 0, 0.3, 1.0, 0, 0);
    constexpr bool JAC = EMUL_RUN_JAC != 0;
#if !EMUL_RUN_JAC
    const int cyl = S.add(DCOL_CYLINDER, 0, 0.3, 1.0, 0, 0);
#endif
    const int p123 = S.polytope(g, 123), p127 = S.polytope(g, 127), p186 = S.polytope(g, 186), p187 = S.polytope(g, 187),
              p192 = S.polytope(g, 192), p511 = S.polytope(g, 511), p512 = S.polytope(g, 512), p512b = S.polytope(g, 512),
              p723 = S.polytope(g, 723);
#if !EMUL_RUN_JAC
    const int p1020 = S.polytope(g, 1020);
#endif
    const int g300 = S.polygon(300, 0.6, 0.2), g1023 = S.polygon(1023, 0.6, 0.2);
#if EMUL_RUN_JAC
    const int pairs[][2] = {{p123, box}, {p186, box}, {p187, box}, {p511, p512}, {p512, p512b},   // (4, 0)
                            {p192, sph},                                                       // (4, 1)
                            {cap, p127},                                                       // (5, 1)
                            {g300, p723},                                                      // (6, 1)
                            {g1023, cone}};                                                    // (6, 2)
    const int modes[] = {DCOL_GRAD_FD | DCOL_CONTACT | DCOL_JACOBIAN, DCOL_CONTACT | DCOL_JACOBIAN};
#else
    const int pairs[][2] = {{p123, box}, {box, p123}, {p127, cap}, {cap, p127},       // 129
                            {p186, box}, {p192, sph}, {sph, p192},                   // 192
                            {p187, box}, {p192, cone}, {cone, p192},                 // 193
                            {p511, p512}, {g300, p723}, {p723, g300},                // 1,023
                            {p512, p512b}, {g1023, cone}, {cone, g1023}, {cyl, p1020}, {p1020, cyl}};   // 1,024
    const int modes[] = {DCOL_GRAD_FD | DCOL_CONTACT, DCOL_GRAD_ENVELOPE | DCOL_CONTACT, DCOL_GRAD_IMPLICIT | DCOL_CONTACT};
#endif
    S.bind();
    const int B = (int)(sizeof(pairs) / sizeof(pairs[0]));
    std::vector<DevShape> sh;
    std::vector<DevRow> rows;
    if (digest_all(S.d.data(), (int32_t)S.d.size(), sh, rows)) {
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
    for (const int flags : modes) {
        std::vector<double> ws = stream_state();   // a fresh one per batch, like a launch's LDS
        const int rc = run_batch(sh, rows, B, s1.data(), s2.data(), p1.data(), p2.data(), 1e-6, 50, flags, alpha.data(),
                                 contact.data(), grad.data(), jac.data(), iters.data(), status.data(),
                                 [&](const KArgs& A, int64_t i) { return stream_pair<JAC>(A, i, ws.data()); });
        if (rc) {
            std::fprintf(stderr, "solve: %s\n", last_error().c_str());
            return 1;
        }
        const int mode = flags & ~(DCOL_CONTACT | DCOL_JACOBIAN);
        for (int i = 0; i < B; ++i) {
            const PairClass c = classify(sh[s1[i]], sh[s2[i]]);
            bool fin = std::isfinite(alpha[i]);
#if EMUL_RUN_JAC
            double jmax = 0.0;
            for (int q = 0; q < 48; ++q) {
                fin = fin && std::isfinite(jac[48 * i + q]);
                jmax = std::fmax(jmax, std::fabs(jac[48 * i + q]));
            }
            std::printf("mode %2d pair %2d (N, NSOC) (%d, %d) rows %4d status %d iters %2d alpha %.12g max|J| %.6g%s\n", mode, i,
                        c.N, c.nsoc, c.o, status[i], iters[i], alpha[i], jmax, fin ? "" : "  NON-FINITE");
#else
            for (int q = 0; q < 3; ++q) fin = fin && std::isfinite(contact[3 * i + q]);
            for (int q = 0; q < 12; ++q) fin = fin && std::isfinite(grad[12 * i + q]);
            std::printf("mode %2d pair %2d rows %4d status %d iters %2d alpha %.12g%s\n", mode, i, c.o, status[i], iters[i],
                        alpha[i], fin ? "" : "  NON-FINITE");
#endif
            bad += !fin || status[i] != DCOL_OK;
        }
    }
    return bad ? 1 : 0;
}
