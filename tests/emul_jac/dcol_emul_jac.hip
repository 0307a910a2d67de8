// TEST-ONLY x86 build of the contact-point Jacobian copies (csrc/dcol_device.hpp: solve_one
// JAC, the dense-row kernels of DCOL_JAC_VARIANTS at one lane per pair), so the Jacobian's
// arithmetic can be checked against its NumPy restatement without a GPU
// (tests/test_contact_jacobian.py).  Built by tests/emul_jac/Makefile into
// tests/emul_jac/libdcol_emul_jac.so: this one source once per primal dimension
// (-DEMUL_JAC_N=4..8: the solver instantiations) and once without (the entry point).
#include <vector>

#include "../../dcol-trajectory-optimization_amd/csrc/dcol_host.hpp"

namespace emul_jac {
using namespace dcol;
using namespace dcol_host;

// Solves pair i of A with the JAC copy of shape (X, nsoc, omax); false if there is none
template <int X>
bool solve_n(int nsoc, int omax, const KArgs& A, int64_t i);

#ifdef EMUL_JAC_N
template <int X>
bool solve_n(int nsoc, int omax, const KArgs& A, int64_t i) {
#define DCOL_EMUL_JAC(NN, NS, OM, LP, WP, FL)                                                              \
    if constexpr (NN == X) {                                                                             \
        if (nsoc == NS && omax == OM) {                                                                  \
            solve_one<NN, NS, OM, 1, false, false, false, 0, 0, false, false, false, false, true>(A, i, 0); \
            return true;                                                                                 \
        }                                                                                                \
    }
    DCOL_JAC_VARIANTS(DCOL_EMUL_JAC)
#undef DCOL_EMUL_JAC
    (void)nsoc; (void)omax; (void)A; (void)i;
    return false;
}
template bool solve_n<EMUL_JAC_N>(int, int, const KArgs&, int64_t);
#endif
}  // namespace emul_jac

#ifndef EMUL_JAC_N
using namespace dcol;
using namespace dcol_host;

// host AoS in and out like dcol_prox_jacobian_host: jac is [B][4][12]
extern "C" int dcol_emul_jac_batch(const dcol_shape_desc* shapes, int32_t n, int64_t B, const int32_t* s1,
                                   const int32_t* s2, const double* pose1, const double* pose2, double tol,
                                   int32_t max_iter, int32_t flags, int32_t case4, double* alpha, double* contact,
                                   double* grad, double* jac, int32_t* iters, int32_t* status) {
    std::vector<DevShape> sh(n);
    std::vector<DevRow> rows;
    init_row_pool(rows);
    for (int32_t i = 0; i < n; ++i) {
        int rc = digest_shape(shapes[i], i, sh[i], rows);
        if (rc) return rc;
    }
    std::vector<double> p1(6 * B), p2(6 * B), ct(3 * B), gr(12 * B), jc(48 * B);
    for (int64_t i = 0; i < B; ++i)
        for (int q = 0; q < 6; ++q) {
            p1[q * B + i] = pose1[6 * i + q];
            p2[q * B + i] = pose2[6 * i + q];
        }
    KArgs A;
    A.shapes = sh.data();
    A.rows = rows.data();
    A.s1 = s1;
    A.s2 = s2;
    A.pose1 = p1.data();
    A.pose2 = p2.data();
    A.perm = nullptr;
    A.B = B;
    A.slot0 = 0;
    A.n = B;
    A.tol = tol;
    A.max_iter = max_iter;
    A.flags = flags | F_JAC;
    A.alpha = alpha;
    A.contact = ct.data();
    A.grad = gr.data();
    A.iters = iters;
    A.status = status;
    A.jac = jc.data();
    const double nan = __builtin_nan("");
    for (int64_t i = 0; i < B; ++i) {
        const PairClass c = classify(sh[s1[i]], sh[s2[i]], case4 != 0, /*part=*/false);   // dense rows
        if (c.status != DCOL_OK) {
            alpha[i] = nan;
            iters[i] = 0;
            status[i] = c.status;
            for (int q = 0; q < 3; ++q) ct[q * B + i] = nan;
            for (int q = 0; q < 12; ++q) gr[q * B + i] = nan;
            for (int q = 0; q < 48; ++q) jc[q * B + i] = nan;
            continue;
        }
        bool done = false;
        switch (c.N) {
            case 4: done = emul_jac::solve_n<4>(c.nsoc, c.omax, A, i); break;
            case 5: done = emul_jac::solve_n<5>(c.nsoc, c.omax, A, i); break;
            case 6: done = emul_jac::solve_n<6>(c.nsoc, c.omax, A, i); break;
            case 7: done = emul_jac::solve_n<7>(c.nsoc, c.omax, A, i); break;
            case 8: done = emul_jac::solve_n<8>(c.nsoc, c.omax, A, i); break;
        }
        if (!done) return fail(DCOL_ERR_ARG, "no JAC copy of the pair's shape");
    }
    for (int64_t i = 0; i < B; ++i) {
        for (int q = 0; q < 3; ++q) contact[3 * i + q] = ct[q * B + i];
        for (int q = 0; q < 12; ++q) grad[12 * i + q] = gr[q * B + i];
        for (int q = 0; q < 48; ++q) jac[48 * i + q] = jc[q * B + i];
    }
    return DCOL_SUCCESS;
}
#endif
