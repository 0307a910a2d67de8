// The streamed-row solve kernels (dcol_device.hpp StreamSolver / prox_stream_kernel): pairs
// of combine cases 1-3 whose orthant rows exceed the register kernels' buckets, up to
// DCOL_MAX_PAIR_ROWS.  One wave per pair, one instance per (N, NSOC) in which a polytope or a
// polygon can bring many rows (DCOL_STREAM_SHAPES); the SOC blocks are dense, so an instance
// serves ball and cone blocks alike.  Launched per bucket by dcol_capi.cpp plan_run_rec.
#include "dcol_device.hpp"
#include "dcol_launch.hpp"

namespace dcol {

hipError_t launch_stream(int N, int nsoc, const KArgs& args, hipStream_t stream) {
#define DCOL_STREAM_CASE(NN, NS)                                                                          \
    if (N == NN && nsoc == NS) {                                                                          \
        hipLaunchKernelGGL((prox_stream_kernel<NN, NS>), dim3((unsigned)args.n), dim3(kStreamBlock), 0, stream, args); \
        return hipGetLastError();                                                                         \
    }
    if (args.n <= 0) return hipSuccess;
    DCOL_STREAM_SHAPES(DCOL_STREAM_CASE)
#undef DCOL_STREAM_CASE
    return hipErrorInvalidValue;
}

DCOL_EXEC_READER(stream)

}  // namespace dcol
