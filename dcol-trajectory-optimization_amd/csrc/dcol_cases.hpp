// dcol_cases.hpp — the compiled variant lists (dcol_variants.inc) as a build sees them: the
// development-build switches applied in one place, for the multi-case kernels
// (dcol_kernels_fused.hip, _packed.hip, _server.hip) and for the case lookups of the plan
// policy (dcol_plan.hpp fused_vid / packed_vid), which must agree on what is compiled.
// Include this instead of dcol_variants.inc wherever the fused or packed lists are read.
#pragma once
#include "dcol_variants.inc"

// Development builds (make dev): no fused cases -- small mixed plans launch per bucket
// (fan-out), dcol_prox_pair launches per call -- and no packed cases, so the multi-case
// units, whose compile time is the sum of their ~100 solver copies, build in seconds.
#ifdef DCOL_NO_FUSED_CASES
#undef DCOL_FUSED_VARIANTS
#define DCOL_FUSED_VARIANTS(X)
#undef DCOL_FUSED_PART_VARIANTS
#define DCOL_FUSED_PART_VARIANTS(X)
#endif
#ifdef DCOL_NO_PACKED_CASES
#undef DCOL_PACKED_VARIANTS
#define DCOL_PACKED_VARIANTS(X)
#endif
