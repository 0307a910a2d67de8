// The streamed-row solve kernels of case-4 pairs (dcol_device.hpp StreamSolver, N >= 7: both
// primitives bring extra primal columns, primitive 2's placed after primitive 1's): polygon x
// capsule / cylinder (7, 2) and polygon x polygon (8, 2) above the register kernels' 32-row
// buckets, up to DCOL_MAX_PAIR_ROWS (DCOL_STREAM_CASE4_SHAPES).  One workgroup of one wave per
// slot and 40 KiB of LDS row state, as dcol_kernels_stream.hip.  Launched per bucket by
// dcol_capi.cpp plan_run_rec for plans made with DCOL_PLAN_CASE4 | DCOL_PLAN_CASE4_STREAM.
#include "dcol_device.hpp"
#include "dcol_launch.hpp"

namespace dcol {

hipError_t launch_stream_c4(int N, int nsoc, const KArgs& args, hipStream_t stream) {
#define DCOL_STREAM_C4_CASE(NN, NS)                                                                       \
    if (N == NN && nsoc == NS) {                                                                          \
        hipLaunchKernelGGL((prox_stream_kernel<NN, NS>), dim3((unsigned)args.n), dim3(kStreamBlock), 0, stream, args); \
        return hipGetLastError();                                                                         \
    }
    if (args.n <= 0) return hipSuccess;
    DCOL_STREAM_CASE4_SHAPES(DCOL_STREAM_C4_CASE)
#undef DCOL_STREAM_C4_CASE
    return hipErrorInvalidValue;
}

DCOL_EXEC_READER(stream_c4)

}  // namespace dcol
