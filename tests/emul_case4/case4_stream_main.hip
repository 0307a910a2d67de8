// TEST-ONLY stand-alone program (its own main, no Python, nothing preloaded): the x86 build of
// the case-4 streamed instances -- StreamSolver<7, 2> and <8, 2> -- on shapes of its own making,
// for a run under the host address and undefined-behaviour sanitizers (tests/emul_case4/Makefile;
// tests/test_case4_stream.py runs it).  The row state is a heap array of exactly the kernel's LDS
// size, the row pool exactly the shapes' rows.  Row totals 33 (the first streamed count: one
// partial slot), 65 (one row over a slot), 1,023 and 1,024 (one short of the cap, the cap), with
// the polygon first and second (primitive 2's extra columns at offset 2 and 1), in the three
// gradient modes on the plain instances and, on the Jacobian copies, with the FD gradient (shared
// z aggregates) and without a gradient.
// Exit status: 0 if every pair converged to finite values, 1 otherwise.
#include <cmath>
#include <cstdio>
#include <vector>

#include "case4_batch.hpp"

namespace {
using namespace emul;

struct Rng {   // splitmix64
    unsigned long long s = 0x2545f4914f6cdd1dull;
    unsigned long long next() {
        unsigned long long z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 11) * (1.0 / 9007199254740992.0)); }
};

struct Shapes {
    std::vector<std::vector<double>> A, b;   // storage the descriptors point into
    std::vector<dcol_shape_desc> d;
    int add(int type, int nh, double R, double L) {
        dcol_shape_desc s{};
        s.type = type;
        s.nh = nh;
        s.R = R;
        s.L = L;
        for (int k = 0; k < 9; ++k) s.Q_offset[k] = (k % 4 == 0) ? 1.0 : 0.0;
        d.push_back(s);
        return (int)d.size() - 1;
    }
    // k-gon with edge normals at jittered angles and offsets U(0.5, 0.9)
    int polygon(Rng& g, int k) {
        std::vector<double> a(2 * k), o(k);
        for (int j = 0; j < k; ++j) {
            const double t = 6.283185307179586 * (j + g.uni(-0.3, 0.3)) / k;
            a[2 * j] = std::cos(t);
            a[2 * j + 1] = std::sin(t);
            o[j] = g.uni(0.5, 0.9);
        }
        A.push_back(a);
        b.push_back(o);
        return add(DCOL_POLYGON, k, 0.2, 0);
    }
    void bind() {   // once every shape is made (the storage vectors no longer grow)
        for (size_t i = 0, k = 0; i < d.size(); ++i)
            if (d[i].nh) {
                d[i].A = A[k].data();
                d[i].b = b[k].data();
                ++k;
            }
    }
};

template <bool JAC>
int run_modes(const std::vector<DevShape>& sh, const std::vector<DevRow>& rows, int B, const int32_t* s1, const int32_t* s2,
              const double* p1, const double* p2, const int* modes, int nmodes) {
    using namespace emul;
    std::vector<int32_t> iters(B), status(B);
    std::vector<double> alpha(B), contact(3 * B), grad(12 * B), jac(48 * B);
    int bad = 0;
    for (int m = 0; m < nmodes; ++m) {
        const int flags = modes[m];
        std::vector<double> ws = stream_state();   // a fresh one per batch, like a launch's LDS
        const int rc = run_batch(sh, rows, B, s1, s2, p1, p2, 1e-6, 50, flags, alpha.data(), contact.data(), grad.data(),
                                 jac.data(), iters.data(), status.data(),
                                 [&](const KArgs& A, int64_t i) { return case4_stream_pair<JAC>(A, i, ws.data()); });
        if (rc) {
            std::fprintf(stderr, "solve: %s\n", last_error().c_str());
            return 1000;
        }
        for (int i = 0; i < B; ++i) {
            const PairClass c = classify(sh[s1[i]], sh[s2[i]], true, false, true, true);
            bool fin = std::isfinite(alpha[i]);
            for (int q = 0; q < 3; ++q) fin = fin && std::isfinite(contact[3 * i + q]);
            if (flags & DCOL_GRAD_ANY)
                for (int q = 0; q < 12; ++q) fin = fin && std::isfinite(grad[12 * i + q]);
            if (JAC)
                for (int q = 0; q < 48; ++q) fin = fin && std::isfinite(jac[48 * i + q]);
            std::printf("jac %d mode %2d pair %2d (N, NSOC) (%d, %d) rows %4d streamed %d status %d iters %2d alpha %.12g%s\n",
                        JAC ? 1 : 0, flags & DCOL_GRAD_ANY, i, c.N, c.nsoc, c.o, c.stream ? 1 : 0, status[i], iters[i], alpha[i],
                        fin ? "" : "  NON-FINITE");
            bad += !fin || status[i] != DCOL_OK || !c.stream;
        }
    }
    return bad;
}
}  // namespace

int main() {
    using namespace emul;
    Rng g;
    Shapes S;
    const int cap = S.add(DCOL_CAPSULE, 0, 0.3, 1.0), cyl = S.add(DCOL_CYLINDER, 0, 0.3, 1.0);
    const int g16 = S.polygon(g, 16), g17 = S.polygon(g, 17), g31 = S.polygon(g, 31), g32 = S.polygon(g, 32),
              g33 = S.polygon(g, 33), g61 = S.polygon(g, 61), g511 = S.polygon(g, 511), g512 = S.polygon(g, 512),
              g512b = S.polygon(g, 512), g1020 = S.polygon(g, 1020), g1021 = S.polygon(g, 1021);
    const int pairs[][2] = {{g31, cap}, {cap, g31}, {g16, g17},                  // 33
                            {g61, cyl}, {cyl, g61}, {g32, g33},                  // 65
                            {g1021, cap}, {cap, g1021}, {g511, g512},            // 1,023
                            {g1020, cyl}, {cyl, g1020}, {g512, g512b}};          // 1,024
    S.bind();
    const int B = (int)(sizeof(pairs) / sizeof(pairs[0]));
    std::vector<DevShape> sh;
    std::vector<DevRow> rows;
    if (digest_all(S.d.data(), (int32_t)S.d.size(), sh, rows)) {
        std::fprintf(stderr, "digest: %s\n", last_error().c_str());
        return 1;
    }
    rows.shrink_to_fit();
    std::vector<int32_t> s1(B), s2(B);
    std::vector<double> p1(6 * B), p2(6 * B);
    for (int i = 0; i < B; ++i) {
        s1[i] = pairs[i][0];
        s2[i] = pairs[i][1];
        for (int q = 0; q < 6; ++q) {
            p1[6 * i + q] = q < 3 ? g.uni(-1.5, 1.5) : g.uni(-1, 1);
            p2[6 * i + q] = q < 3 ? g.uni(-1.5, 1.5) : g.uni(-1, 1);
        }
    }
    const int plain[] = {DCOL_GRAD_FD | DCOL_CONTACT, DCOL_GRAD_ENVELOPE | DCOL_CONTACT, DCOL_GRAD_IMPLICIT | DCOL_CONTACT};
    const int withjac[] = {DCOL_GRAD_FD | DCOL_CONTACT | DCOL_JACOBIAN, DCOL_CONTACT | DCOL_JACOBIAN};
    int bad = run_modes<false>(sh, rows, B, s1.data(), s2.data(), p1.data(), p2.data(), plain, 3);
    bad += run_modes<true>(sh, rows, B, s1.data(), s2.data(), p1.data(), p2.data(), withjac, 2);
    return bad ? 1 : 0;
}
