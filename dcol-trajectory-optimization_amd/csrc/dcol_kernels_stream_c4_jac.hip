// The case-4 streamed kernels' contact-point Jacobian copies (dcol_device.hpp solve_stream JAC):
// one instance per DCOL_STREAM_CASE4_SHAPES, for the streamed case-4 pairs of a plan made with
// DCOL_PLAN_CASE4 | DCOL_PLAN_CASE4_STREAM | DCOL_PLAN_JACOBIAN | DCOL_PLAN_JACOBIAN_STREAM.  Same
// solve and gradient as the plain instances (dcol_kernels_stream_c4.hip), bitwise; the Jacobian
// phase runs after them.  Launched per bucket by dcol_capi.cpp plan_run_rec for runs with
// DCOL_JACOBIAN only.
#include "dcol_device.hpp"
#include "dcol_launch.hpp"

namespace dcol {

hipError_t launch_stream_c4_jac(int N, int nsoc, const KArgs& args, hipStream_t stream) {
#define DCOL_STREAM_C4_JAC_CASE(NN, NS)                                                                         \
    if (N == NN && nsoc == NS) {                                                                                \
        hipLaunchKernelGGL((prox_stream_kernel<NN, NS, true>), dim3((unsigned)args.n), dim3(kStreamBlock), 0, stream, \
                           args);                                                                               \
        return hipGetLastError();                                                                               \
    }
    if (args.n <= 0) return hipSuccess;
    DCOL_STREAM_CASE4_SHAPES(DCOL_STREAM_C4_JAC_CASE)
#undef DCOL_STREAM_C4_JAC_CASE
    return hipErrorInvalidValue;
}

DCOL_EXEC_READER(stream_c4_jac)

}  // namespace dcol
