// The JAC copies: the dense-row solve kernel with the contact-point Jacobian phase
// (dcol_device.hpp solve_one JAC, Solver::jacobian_factor / jacobian_adjoints), one per shape
// of dcol_variants.inc DCOL_JAC_VARIANTS (variants.py jac()).  Launched for the buckets of a
// DCOL_PLAN_JACOBIAN plan by a run with DCOL_JACOBIAN (dcol_capi.cpp dcol_plan_run_jac).
// One source, one object per primal dimension (-DDCOL_JAC_N=4..8, csrc/Makefile), so the
// copies compile side by side like the per-N units of the solve kernels.
#include "dcol_device.hpp"
#include "dcol_launch.hpp"
#include "dcol_variants.inc"

#ifndef DCOL_JAC_N
#error "compile with -DDCOL_JAC_N=<primal dimension, 4..8>"
#endif
#define DCOL_JAC_CAT_(a, b) a##b
#define DCOL_JAC_CAT(a, b) DCOL_JAC_CAT_(a, b)

namespace dcol {

#define DCOL_CASE(NN, NS, OM, LP, WP, FL)                                                       \
    if constexpr (NN == DCOL_JAC_N)                                                           \
        if (nsoc == NS && omax == OM && lpp == LP) {                                           \
            const int64_t grid = solve_grid(args, LP);   /* (the run passes no order hint) */  \
            hipLaunchKernelGGL((prox_kernel<NN, NS, OM, LP, WP, FL, 0, true>), dim3(grid), dim3(kBlock), 0, stream, args); \
            return hipGetLastError();                                                         \
        }

hipError_t DCOL_JAC_CAT(launch_jac_n, DCOL_JAC_N)(int nsoc, int omax, int lpp, const KArgs& args, hipStream_t stream) {
    DCOL_JAC_VARIANTS(DCOL_CASE)
    return hipErrorInvalidValue;
}

#define DCOL_JAC_READER(tag) DCOL_EXEC_READER(tag)
DCOL_JAC_READER(DCOL_JAC_CAT(jac, DCOL_JAC_N))

}  // namespace dcol
