// The streamed-row kernels' contact-point Jacobian copies (dcol_device.hpp solve_stream JAC,
// StreamSolver::jacobian_factor / aggregates<JACW>): one instance per streamed (N, NSOC)
// (DCOL_STREAM_SHAPES), for the pairs of 129 to DCOL_MAX_PAIR_ROWS orthant rows of a plan made
// with DCOL_PLAN_JACOBIAN | DCOL_PLAN_JACOBIAN_STREAM.  Same solve and gradient as the plain
// instances (dcol_kernels_stream.hip), bitwise; the Jacobian phase runs after them.  Launched
// per bucket by dcol_capi.cpp plan_run_rec for runs with DCOL_JACOBIAN only.
#include "dcol_device.hpp"
#include "dcol_launch.hpp"

namespace dcol {

hipError_t launch_stream_jac(int N, int nsoc, const KArgs& args, hipStream_t stream) {
#define DCOL_STREAM_JAC_CASE(NN, NS)                                                                            \
    if (N == NN && nsoc == NS) {                                                                                \
        hipLaunchKernelGGL((prox_stream_kernel<NN, NS, true>), dim3((unsigned)args.n), dim3(kStreamBlock), 0, stream, \
                           args);                                                                               \
        return hipGetLastError();                                                                               \
    }
    if (args.n <= 0) return hipSuccess;
    DCOL_STREAM_SHAPES(DCOL_STREAM_JAC_CASE)
#undef DCOL_STREAM_JAC_CASE
    return hipErrorInvalidValue;
}

DCOL_EXEC_READER(stream_jac)

}  // namespace dcol
