// TEST-ONLY (tests/emul_case4): run_batch's solve of the case-4 streamed instances, shared by the
// library (case4_emul.hip) and the stand-alone sanitizer program (case4_stream_main.hip).
#pragma once
#include "../emul/emul_batch.hpp"

namespace emul {

// solve_stream<7 | 8, 2> at LANES = 1 (JAC: the contact-point Jacobian copies) for every pair
// that classify() accepts under DCOL_PLAN_CASE4 | DCOL_PLAN_CASE4_STREAM (jac: as a Jacobian plan
// with DCOL_PLAN_JACOBIAN_STREAM classifies: no row partition) and whose (N, NSOC) is a case-4
// streamed shape -- whether it is marked streamed or a register bucket would take it.  ws:
// stream_state().
template <bool JAC>
int case4_stream_pair(const KArgs& A, int64_t i, double* ws) {
    const PairClass c = JAC ? classify(A.shapes[A.s1[i]], A.shapes[A.s2[i]], true, /*part=*/false, /*stream=*/true, true)
                            : classify(A.shapes[A.s1[i]], A.shapes[A.s2[i]], true, !part_disabled(), /*stream=*/true, true);
    if (c.status != DCOL_OK) return c.status;
#define EMUL_C4_CASE(NN, NS)                         \
    if (c.N == NN && c.nsoc == NS) {                 \
        solve_stream<NN, NS, 1, JAC>(A, i, 0, ws);   \
        return DCOL_OK;                              \
    }
    DCOL_STREAM_CASE4_SHAPES(EMUL_C4_CASE)
#undef EMUL_C4_CASE
    return fail(DCOL_ERR_ARG, "pair " + std::to_string(i) + ": no case-4 streamed instance for its (N, NSOC)");
}

}  // namespace emul
