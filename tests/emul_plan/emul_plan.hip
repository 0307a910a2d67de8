// TEST-ONLY x86 build of the plan policy (csrc/dcol_plan.hpp: dcol_host::plan_layout), for
// tests/test_plan_layout.py (tests/emul_plan/libdcol_plan_emul.so): what a plan would launch,
// without a device.
#include <cstring>
#include <vector>

#include "../../dcol-trajectory-optimization_amd/csrc/dcol_plan.hpp"

using namespace dcol;
using namespace dcol_host;

// The layout of the plan of pairs (s1[i], s2[i]), i < B, over the shapes (the descriptors
// dcol_table_create takes) on a device with `simds` SIMDs.  options: DCOL_PLAN_CASE4 |
// DCOL_PLAN_NO_FUSE.  policy: the PlanPolicy fields in declaration order (clamped here like
// from_env's).  Out, for at most max_buckets buckets: info / pairs as dcol_plan_bucket gives
// them and each bucket's stream (lane); head = {buckets, launch form, streams, launches (the
// three as the dcol_plan_* getters compute them), lanes, small, segments, fused_blocks,
// issue entries}; perm[B]; issue; segs rows {vid, lpp, block0, slot0, n}.  On an error its
// message is copied to err.
extern "C" int dcol_emul_plan(const dcol_shape_desc* shapes, int32_t n, int32_t simds, int64_t B, const int32_t* s1,
                              const int32_t* s2, int32_t options, const int64_t policy[11], int32_t max_buckets,
                              int32_t* info, int64_t* pairs, int32_t* lane, int64_t head[9], int32_t* perm,
                              int32_t* issue, int64_t* segs, char* err, int32_t errlen) {
    const auto done = [&](int rc) {
        if (rc != DCOL_SUCCESS && err && errlen > 0) {
            std::strncpy(err, last_error().c_str(), (size_t)errlen - 1);
            err[errlen - 1] = 0;
        }
        return rc;
    };
    std::vector<DevShape> sh(n);
    std::vector<DevRow> rows;
    init_row_pool(rows);
    for (int32_t i = 0; i < n; ++i) {
        const int rc = digest_shape(shapes[i], i, sh[i], rows);
        if (rc != DCOL_SUCCESS) return done(rc);
    }
    PlanPolicy pol;
    pol.no_ball = policy[0] != 0;
    pol.no_box = policy[1] != 0;
    pol.no_cone = policy[2] != 0;
    pol.small_plan_lanes = policy[3];
    pol.pack_lanes = policy[4];
    pol.small_fanout = policy[5] != 0;
    pol.latency_per_launch = policy[6] != 0;
    pol.no_fanout = policy[7] != 0;
    pol.fused_key_order = policy[8] != 0;
    pol.side_streams = (int)policy[9];
    pol.side_streams_large = (int)policy[10];
    pol.clamp();
    PlanLayout p;
    const int rc = plan_layout(sh, simds, B, s1, s2, (options & DCOL_PLAN_CASE4) != 0, (options & DCOL_PLAN_NO_FUSE) == 0,
                               pol, p);
    if (rc != DCOL_SUCCESS) return done(rc);
    if ((int64_t)p.buckets.size() > max_buckets) return done(fail(DCOL_ERR_ARG, "dcol_emul_plan: more buckets than max_buckets"));
    int64_t launches = 0;
    for (size_t i = 0; i < p.buckets.size(); ++i) {
        const Bucket& L = p.buckets[i];
        const bool solve = L.kind == 0;
        const int32_t v[8] = {L.kind, solve ? L.N : 0, solve ? L.nsoc : 0, solve ? L.omax : 0, solve ? L.lpp : 0,
                              solve ? L.oe : 0, solve ? L.flags() : 0, solve ? 0 : L.code};
        std::memcpy(info + 8 * i, v, sizeof(v));
        pairs[i] = L.n;
        lane[i] = L.lane;
        launches += (L.kind != 0 || !p.fused());
    }
    head[0] = (int64_t)p.buckets.size();
    head[1] = !p.fused() ? DCOL_FORM_BUCKETS : (p.packed ? DCOL_FORM_PACKED : DCOL_FORM_FUSED);
    head[2] = p.fused() ? 1 : p.lanes;
    head[3] = launches + (p.fused() ? 1 : 0);
    head[4] = p.lanes;
    head[5] = p.small;
    head[6] = (int64_t)p.segs.size();
    head[7] = p.fused_blocks;
    head[8] = (int64_t)p.issue.size();
    if (B > 0) std::memcpy(perm, p.perm.data(), sizeof(int32_t) * (size_t)B);
    for (size_t i = 0; i < p.issue.size(); ++i) issue[i] = p.issue[i];
    for (size_t i = 0; i < p.segs.size(); ++i) {
        const FusedSeg& S = p.segs[i];
        const int64_t v[5] = {S.vid, S.lpp, S.block0, S.slot0, S.n};
        std::memcpy(segs + 5 * i, v, sizeof(v));
    }
    return DCOL_SUCCESS;
}
