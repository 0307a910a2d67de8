// Row-partitioned (PART) kernel instantiations of one (N, NSOC) pair, included by
// dcol_kernels_p<N><NSOC>.hip (one translation unit each, so the variants compile in
// parallel).  Variant list: DCOL_PART_VARIANTS in dcol_variants.inc (variants.py).
#include <cstdlib>

#include "dcol_device.hpp"
#include "dcol_launch.hpp"
#include "dcol_variants.inc"

namespace dcol {

// list order per bucket: FULL|BALL, BALL, FULL, dense -- the first whose flags the launch
// allows is taken (as the per-N launchers do).  DCOL_WPS=<w> (A/B runs): copies built for w
// waves per SIMD first (variants.py lists a bucket's (LPP, WPS) alternatives); a bucket with
// no such copy takes its default one
// DCOL_TU_FLOK(FL): the unit's share of the (N, NSOC) variants by flavour (default all; the
// N = 6, NSOC = 2 variants are split into a ball-row unit and a dense-row unit, each under its
// own machine schedule, Makefile SCHED_XPOLY)
#ifndef DCOL_TU_FLOK
#define DCOL_TU_FLOK(FL) true
#endif
#define DCOL_PCASE(NN, NS, OM, LP, WP, FL, OEE)                                                    \
    if constexpr (NN == DCOL_TU_N && NS == DCOL_TU_NS && DCOL_TU_FLOK(FL))                         \
        if (omax == OM && oe == OEE && lpp == LP && (FL & flags) == FL && (wps == 0 || wps == WP % 10)) { \
            const int64_t grid = solve_grid(args, LP);                                             \
            hipLaunchKernelGGL((prox_kernel<NN, NS, OM, LP, WP, FL, OEE>), dim3(grid), dim3(kBlock), 0, stream, args); \
            return hipGetLastError();                                                              \
        }

namespace {
// one pass over the bucket's copies; wps 0: no filter.  hipErrorInvalidValue: none matched
// (a function called twice, not a loop around the list: the host compiler took an hour
// over the loop form)
__attribute__((noinline)) hipError_t part_pass(int omax, int oe, int lpp, int flags, int wps, const KArgs& args,
                                                  hipStream_t stream) {
    DCOL_SPLIT_VARIANTS(DCOL_PCASE)   // (launch flag LF_SPLIT: the split-SOC copies first)
    DCOL_PART_VARIANTS(DCOL_PCASE)
    (void)omax; (void)oe; (void)lpp; (void)flags; (void)wps; (void)args; (void)stream;
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t DCOL_TU_FN(int omax, int oe, int lpp, int flags, const KArgs& args, hipStream_t stream) {
    static const int wps = [] {
        const char* e = std::getenv("DCOL_WPS");
        return e ? std::atoi(e) : 0;
    }();
    const hipError_t e = part_pass(omax, oe, lpp, flags, wps, args, stream);
    return (e == hipErrorInvalidValue && wps != 0) ? part_pass(omax, oe, lpp, flags, 0, args, stream) : e;
}

#define DCOL_EXEC_READER_X(t) DCOL_EXEC_READER(t)   // expand DCOL_TU_TAG before pasting
DCOL_EXEC_READER_X(DCOL_TU_TAG)

}  // namespace dcol
