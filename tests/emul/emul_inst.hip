// TEST-ONLY (tests/emul): one object's share of the x86 solver instantiations, chosen by the
// Makefile: -DEMUL_N=.. -DEMUL_NS=.. the dense-row dispatch of one (N, NSOC) (with
// -DEMUL_NO_PART_SHAPES=1 also the empty PART one of a combination without PART buckets),
// plus -DEMUL_PART=1 the row-partitioned buckets' dispatch instead; -DEMUL_JAC_N=.. the
// contact-point Jacobian copies of one N; -DEMUL_STREAM_JAC=0 / 1 the streamed-row solver /
// its Jacobian copies.
#include "emul_solve.hpp"

#if defined(EMUL_STREAM_JAC)
template int emul::stream_pair<EMUL_STREAM_JAC != 0>(const dcol::KArgs&, int64_t, double*);
#elif defined(EMUL_JAC_N)
template bool emul::solve_jac<EMUL_JAC_N>(int, int, const dcol::KArgs&, int64_t);
#elif EMUL_PART
template bool emul::solve_part<EMUL_N, EMUL_NS>(const dcol_host::PairClass&, bool, bool, const dcol::KArgs&, int64_t);
#else
template bool emul::solve_n<EMUL_N, EMUL_NS>(const dcol_host::PairClass&, bool, bool, bool, bool, const dcol::KArgs&, int64_t);
#if EMUL_NO_PART_SHAPES
template bool emul::solve_part<EMUL_N, EMUL_NS>(const dcol_host::PairClass&, bool, bool, const dcol::KArgs&, int64_t);
#endif
#endif
