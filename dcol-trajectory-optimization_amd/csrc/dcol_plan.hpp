// dcol_plan.hpp — the plan policy: which kernel copy, lane count, launch form and stream each
// pair of a batch gets, as a function of plain values (shape digests, the device's SIMD
// count, the pair lists, a PlanPolicy).  Host arithmetic only: no HIP runtime call, no device
// state.  Shared by the C-ABI (dcol_capi.cpp: dcol_plan_create_ex, dcol_prox_batch_host, the
// one-pair plans of dcol_prox_pair) and its test-only x86 build (tests/emul_plan,
// tests/test_plan_layout.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

#include "dcol_host.hpp"
#include "dcol_launch.hpp"
#include "dcol_cases.hpp"

namespace dcol_host {

// Fused variant id of a kernel shape + (lpp, launch flags, PART extra slots oe), or -1 if the
// fused kernel (dcol_kernels_fused.hip; the pair server switches over the same cases) lacks
// it.  A bucket whose pairs all fill OMAX takes the padding-free case if there is one, a
// bucket of ball-SOC or cone-SOC pairs the structured case, else the plain one -- as the
// per-variant launchers do.
inline int fused_vid(int N, int nsoc, int omax, int lpp, int flags, int oe = 0) {
    if (oe > 0) {   // row-partitioned bucket: FULL|BALL, BALL, FULL, dense
        for (const int want : {(int)(LF_FULL | LF_BALL), (int)LF_BALL, (int)LF_FULL, 0}) {
            if ((want & flags) != want) continue;
#define DCOL_FPID(ID, NN, NS, OM, LP, FL, OEE) \
    if (NN == N && NS == nsoc && OM == omax && OEE == oe && LP == lpp && FL == want) return ID;
            DCOL_FUSED_PART_VARIANTS(DCOL_FPID)
#undef DCOL_FPID
        }
        return -1;
    }
    for (const int want : {(int)LF_FULL, (int)LF_BALL, (int)LF_CONE, 0}) {
        if ((want & flags) != want) continue;
#define DCOL_FID(ID, NN, NS, OM, LP, FL) \
    if (NN == N && NS == nsoc && OM == omax && LP == lpp && FL == want) return ID;
        DCOL_FUSED_VARIANTS(DCOL_FID)
#undef DCOL_FID
    }
    (void)N; (void)nsoc; (void)omax; (void)lpp;
    return -1;
}

// Packed case id (dcol_kernels_packed.hip) of a bucket: the first entry of its shape (and
// LPP) whose flavour the bucket's launch flags allow -- the list is in the per-variant
// launchers' preference order -- or -1
inline int packed_vid(int N, int nsoc, int omax, int lpp, int flags, int oe = 0) {
#define DCOL_KID(ID, NN, NS, OM, LP, FL, OEE) \
    if (NN == N && NS == nsoc && OM == omax && LP == lpp && OEE == oe && (FL & flags) == FL) return ID;
    DCOL_PACKED_VARIANTS(DCOL_KID)
#undef DCOL_KID
    (void)N; (void)nsoc; (void)omax; (void)lpp; (void)flags; (void)oe;
    return -1;
}

// Every knob of the policy (A/B runs, tests), with its default.  The variables dcol_host.hpp
// reads itself -- DCOL_LPP, DCOL_NO_PART, DCOL_SPLIT, shared with the solver's x86 build --
// stay there.
struct PlanPolicy {
    bool no_ball = false;   // DCOL_NO_BALL (set): ball-SOC pairs run the dense kernels too
    bool no_box = false;    // DCOL_NO_BOX (set): box x box pairs run the padding-free dense-row kernel
    bool no_cone = false;   // DCOL_NO_CONE (set): cone-SOC pairs run the dense (padded) kernels
    // DCOL_SMALL_PLAN_LANES=<n>: lanes below which a plan counts as small -- it cannot fill the
    // GPU: every bucket takes its latency configuration and a mixed plan runs as one fused
    // launch.  0 (default): 64 x SIMDs, one wave per SIMD.
    int64_t small_plan_lanes = 0;
    // DCOL_PACK_LANES=<n>: lanes below which a plan that is not small runs as ONE packed launch
    // (every bucket in its throughput configuration, dcol_kernels_packed.hip) instead of one
    // launch per bucket over the fan-out streams: mid-size mixed plans whose buckets each cover
    // only part of the SIMDs (a rank's shard of configs[4] at 2-8 GPUs).  0: never; negative
    // (default): 16 x 64 x SIMDs (~1M lanes), measured on the configs[4] shards
    // (tools/shard_bench.py, profiles/r06_c/): packed against the fan-out 0.506 / 0.549 ms at
    // 500k pairs (775k lanes), 0.267 / 0.396 at 250k, 0.144 / 0.325 at 125k, but 0.98 / 0.87 ms
    // for the whole 1M (1.55M lanes: every bucket fills the GPU by itself and its two- and
    // three-wave kernels keep their occupancy).
    int64_t pack_lanes = -1;
    // DCOL_SMALL_FANOUT (set): a small plan the fused kernel cannot take fans its
    // latency-configured buckets out (the behaviour before the packed launch)
    bool small_fanout = false;
    // DCOL_LATENCY_PER_LAUNCH (set): a bucket too small to fill the GPU takes its latency
    // configuration even in a plan that fills it (the per-launch rule)
    bool latency_per_launch = false;
    bool no_fanout = false;         // DCOL_NO_FANOUT (set): every launch on the caller's stream
    bool fused_key_order = false;   // DCOL_FUSED_ORDER=0: segments in bucket (key) order, not by cost
    // DCOL_SIDE_STREAMS=<1..kSideStreams>: side streams per device; 3 (with the caller's
    // stream, 4 = HIP's default hardware queues; raise GPU_MAX_HW_QUEUES to match a larger value)
    int side_streams = 3;
    // DCOL_SIDE_STREAMS_LARGE=<1..side_streams>: side streams a plan that fills the GPU fans
    // out over: 2 -- three buckets in flight with the caller's stream.  Fewer concurrent
    // buckets finish a large mixed step sooner: the one-wave-per-SIMD kernels (400-500
    // registers) need a whole SIMD's register file and wait behind co-running buckets' waves
    // when four run at once (1M mixed plan, synchronised steps: 0.87 ms at 2 against 0.94 ms
    // at 3 and 1).  A small plan (its buckets cannot fill the GPU, each
    // runs its latency configuration) keeps every side stream.
    int side_streams_large = 2;

    // the stream counts into their ranges
    void clamp() {
        side_streams = std::min(std::max(side_streams, 1), kSideStreams);
        side_streams_large = std::min(std::max(side_streams_large, 1), side_streams);
    }
    static PlanPolicy from_env() {
        PlanPolicy p;
        const auto set = [](const char* k) { return std::getenv(k) != nullptr; };
        p.no_ball = set("DCOL_NO_BALL");
        p.no_box = set("DCOL_NO_BOX");
        p.no_cone = set("DCOL_NO_CONE");
        if (const char* e = std::getenv("DCOL_SMALL_PLAN_LANES")) p.small_plan_lanes = std::atoll(e);
        if (const char* e = std::getenv("DCOL_PACK_LANES")) p.pack_lanes = std::atoll(e);
        p.small_fanout = set("DCOL_SMALL_FANOUT");
        p.latency_per_launch = set("DCOL_LATENCY_PER_LAUNCH");
        p.no_fanout = set("DCOL_NO_FANOUT");
        if (const char* e = std::getenv("DCOL_FUSED_ORDER")) p.fused_key_order = std::atoi(e) == 0;
        if (const char* e = std::getenv("DCOL_SIDE_STREAMS")) p.side_streams = std::atoi(e);
        if (const char* e = std::getenv("DCOL_SIDE_STREAMS_LARGE")) p.side_streams_large = std::atoi(e);
        p.clamp();
        return p;
    }
    int64_t small_lanes(int simds) const { return small_plan_lanes > 0 ? small_plan_lanes : 64LL * simds; }
    int64_t pack_limit(int simds) const { return pack_lanes >= 0 ? pack_lanes : 16LL * 64LL * simds; }
};

// One launch of a plan, or one segment of its fused / packed launch: a kernel variant, its
// lanes per pair and the plan slots [slot0, slot0 + n) it covers.
struct Bucket {
    int kind = 0;       // 0 = solve, 1 = reject
    int N = 0, nsoc = 0, omax = 0, lpp = 0;
    int oe = 0;          // row-partitioned bucket (extra-row slots; 0: dense-row kernels)
    bool full = false;   // every pair has o == omax: the padding-free kernel (DCOL_FULL_VARIANTS) if built
    bool ball = false;   // every SOC block is a ball block: the structured kernel (DCOL_BALL_VARIANTS) if built
    bool cone = false;   // every SOC block is a cone block (N = 4): DCOL_CONE_VARIANTS if built
    bool box = false;    // every pair is box x box (DevShape::boxp; with full): DCOL_BOX_VARIANTS if built
    int flags() const { return (full ? LF_FULL : 0) | (ball ? LF_BALL : 0) | (cone ? LF_CONE : 0) | (box ? LF_BOX : 0); }
    int32_t code = 0;   // reject status
    int64_t slot0 = 0, n = 0;
    int lane = 0;   // 0 = caller's stream, 1..kSideStreams = side stream
    // streamed bucket (PairClass::stream): the (N, nsoc) streamed-row kernel, a wave per pair
    // (omax = DCOL_MAX_PAIR_ROWS, lpp = 64, dense SOC rows); its slots are in descending row
    // count, and `rows` is the sum of its pairs' row counts rounded up to whole slots
    // (bucket_cost)
    bool stream = false;
    int64_t rows = 0;
};

// What a plan will launch.
struct PlanLayout {
    std::vector<Bucket> buckets;   // in key order (BucketKey)
    std::vector<int32_t> perm;     // plan slot -> pair
    std::vector<int> issue;        // launch issue order (assign_lanes: longest first); empty = as built
    int lanes = 1;                 // streams the launches are spread over (1 = serial)
    bool small = false;            // the plan cannot fill the GPU (bucket_pairs)
    // fused launch (small mixed plans) or packed launch (mid-size plans, packed = true): one
    // segment per solve bucket, in descending per-pair cost (plan_segments)
    std::vector<FusedSeg> segs;
    int64_t fused_blocks = 0;
    bool packed = false;
    bool fused() const { return !segs.empty(); }
};

// SOC form of a bucket's pairs: every block a ball (BALL kernels), every block a cone and
// N = 4 (CONE kernels), or -- without SOC blocks -- box x box in the 12-row bucket (the BOX
// kernels' axis-pair rows); else dense
enum class SocForm { Dense = 0, Ball = 1, Cone = 2, Box = 3 };

// What pairs of one bucket share; buckets are laid out in this order.
struct BucketKey {
    int kind, N, nsoc, omax, lpp;
    SocForm soc;
    int code, oe;
    int stream = 0;   // 1: the streamed bucket of (N, nsoc), after its register buckets
    bool operator<(const BucketKey& o) const {
        return std::tie(kind, N, nsoc, omax, lpp, soc, code, oe, stream) <
               std::tie(o.kind, o.N, o.nsoc, o.omax, o.lpp, o.soc, o.code, o.oe, o.stream);
    }
};

// How bucket_pairs places the pairs (plan_layout's retries)
struct BucketMode {
    bool case4 = false;   // DCOL_PLAN_CASE4
    // a row-partitioned bucket is used only where the fused small-plan kernel has its case
    // (the retry of a small plan that would otherwise lose its single fused launch; the other
    // pairs take the dense-row kernels, which the fused kernel covers)
    bool fused_part = false;
    // a row-partitioned bucket compiled only for one lane per pair is not used (the retry of a
    // plan that cannot fill the GPU: one lane working through every row of the pair is slower
    // than the dense rows' multi-lane groups -- polygon x box, 1,000 pairs: 84 us in the
    // (11, 5) one-lane bucket against 52 us in the dense (6, 1, 12) four-lane kernel)
    bool lat_part = false;
    // bucket as a plan that fills the GPU (throughput configurations: the packed launch of a
    // small plan the fused kernel cannot take)
    bool force_large = false;
    // DCOL_PLAN_JACOBIAN: every pair on the dense-row kernels (no row partition, no ball /
    // cone / box form, whatever the policy says) at the lanes per pair of its shape's
    // Jacobian copy (jac_lpp); set together with force_large (plan_layout_jac)
    bool jac = false;
    // DCOL_PLAN_JACOBIAN_STREAM (with jac): pairs of cases 1-3 above the dense-row buckets, up
    // to DCOL_MAX_PAIR_ROWS rows, are classified streamed as in a plain plan and run the
    // streamed kernels' Jacobian copies; without it they stay DCOL_TOO_LARGE
    bool jac_stream = false;
    // DCOL_PLAN_CASE4_STREAM (with case4): case-4 pairs above their register buckets, up to
    // DCOL_MAX_PAIR_ROWS rows, are classified streamed (classify's case4_stream) and get a
    // streamed bucket per (7, 2) / (8, 2); in a Jacobian plan only with jac_stream as well
    bool case4_stream = false;
};

// A launch too small to fill the GPU runs the configuration with the shortest per-pair
// latency: fewest orthant slots per lane (omax / lpp), over the pair's bucket and the larger
// buckets up to twice its rows (a tight bucket compiled only with LPP 2 -- 6 or 10 rows --
// loses to the next bucket's 8-lane groups), fewer rows on ties.
inline void latency_config(Bucket& L) {
    if (L.stream) return;   // one configuration: a wave per pair
    if (L.oe > 0) {   // row-partitioned bucket: its largest compiled LPP
        L.lpp = part_lpp(L.N, L.nsoc, L.omax, L.oe, /*latency=*/true);
        return;
    }
    const int fl = L.ball ? 2 : (L.cone ? 4 : 0);
    int best_o = L.omax, best_l = max_lpp(L.N, L.nsoc, L.omax, fl);
    for (const int om : buckets().at({L.N, L.nsoc})) {
        if (om <= L.omax || om > 2 * L.omax) continue;
        const int l = max_lpp(L.N, L.nsoc, om, fl);
        if (om * best_l < best_o * l) {   // om / l < best_o / best_l
            best_o = om;
            best_l = l;
        }
    }
    if (best_o != L.omax) L.full = false;   // the pairs no longer fill the bucket
    L.omax = best_o;
    L.lpp = best_l;
}

// Per-pair cost of a solve bucket in ns at full occupancy (least-squares fit to the class
// benchmark of profiles/r03_soc/class_bench.log, within ~17 % on the 13 SOC classes): row
// slots, SOC blocks (dense SOC rows cost more than the structured ball / cone rows) and the
// N x N normal-matrix work; polytope x polytope buckets run at two waves per SIMD (x 0.5).
// A streamed bucket: the same per-row-slot and per-block terms over its pairs' own row counts
// (Bucket::rows) instead of n * omax, the row term doubled -- its rows are re-formed from
// their descriptors in each of the iteration's four passes and it runs one wave per SIMD --
// and the N x N term times 64, since the normal-matrix work a register kernel's lane does for
// its own pair occupies a whole wave here.  An estimate from the kernel's structure, used
// only to order and spread launches.
inline double bucket_cost(const Bucket& L) {
    if (L.stream)
        return 2.0 * 0.0806 * (double)L.rows + (double)L.n * 64.0 * (0.27 * L.nsoc + 0.0139 * L.N * L.N);
    const bool dense_soc = L.nsoc > 0 && !(L.flags() & (LF_BALL | LF_CONE));
    const double per_pair = 0.0806 * L.omax + 0.127 * L.nsoc + 0.0139 * L.N * L.N + (dense_soc ? 0.143 * L.nsoc : 0.0);
    return (double)L.n * per_pair * (L.nsoc == 0 ? 0.5 : 1.0);
}

// Mixed batches (e.g. an ALTRO phase: one victim against spheres, cylinders, capsules,
// cones, polytopes) split into several small variant launches, each far too small to fill
// the chip; run back to back their latencies add up.  Spread them over the caller's stream
// plus the side streams (fork/join through events) -- longest-first greedy on bucket_cost
// (waves x per-pair work), reject launches stay on the caller's stream.
inline void assign_lanes(PlanLayout& p, const PlanPolicy& pol) {
    int solves = 0;
    for (const Bucket& L : p.buckets) solves += L.kind == 0;
    p.lanes = 1;
    p.issue.clear();
    if (solves < 2) return;
    const int lanes = std::min(solves, (p.small ? pol.side_streams : pol.side_streams_large) + 1);
    std::vector<int> order;
    std::vector<double> cost(p.buckets.size(), 0.0);
    for (size_t i = 0; i < p.buckets.size(); ++i) {
        const Bucket& L = p.buckets[i];
        if (L.kind != 0) {
            p.issue.push_back((int)i);   // rejects first, on the caller's stream
            continue;
        }
        cost[i] = bucket_cost(L);
        order.push_back((int)i);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    // issued longest first: every stream starts on its biggest bucket and the short ones fill
    // the tail, where the other streams' last kernels no longer occupy the whole chip
    p.issue.insert(p.issue.end(), order.begin(), order.end());
    std::vector<double> load(lanes, 0.0);
    for (int i : order) {
        const int l = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        p.buckets[i].lane = l;
        load[l] += cost[i];
    }
    p.lanes = pol.no_fanout ? 1 : lanes;
}

// Classify + bucket (counting sort by BucketKey).  Fills p.buckets, p.perm, p.small and the
// lanes; returns DCOL_SUCCESS or an error (p untouched).
// O(B): each distinct (shape1, shape2) is classified once (a dense S x S cache when S^2 is
// at most 4M cells and small against B, else a hash map), then a stable counting sort by
// group, groups in key order.
inline int bucket_pairs(const std::vector<DevShape>& shapes, int simds, int64_t B, const int32_t* s1,
                        const int32_t* s2, const BucketMode& mode, const PlanPolicy& pol, PlanLayout& p) {
    const int32_t ns = (int32_t)shapes.size();
    struct Group {
        BucketKey key;
        bool full = true;   // every pair class of the group has o == omax
        int64_t n = 0, at = 0;
    };
    std::map<BucketKey, int32_t> gid_of_key;
    std::vector<Group> groups;
    auto classify_pair = [&](int32_t i1, int32_t i2) -> int32_t {
        const DevShape& a = shapes[i1];
        const DevShape& b = shapes[i2];
        // (a Jacobian plan's pairs above the buckets stay DCOL_TOO_LARGE unless it opted into
        // the streamed Jacobian copies: BucketMode::jac_stream)
        PairClass c = mode.jac ? classify(a, b, mode.case4, /*part=*/false, /*stream=*/mode.jac_stream, mode.case4_stream)
                               : classify(a, b, mode.case4, !part_disabled(), /*stream=*/true, mode.case4_stream);
        if (mode.jac && c.status == DCOL_OK && !c.stream) c.lpp = jac_lpp(c.N, c.nsoc, c.omax);
        const bool none_cone = a.soc_kind != SOC_CONE && b.soc_kind != SOC_CONE;
        const bool all_cone = a.soc_kind != SOC_BALL && b.soc_kind != SOC_BALL;
        if (mode.fused_part && c.status == DCOL_OK && c.oe > 0 &&
            fused_vid(c.N, c.nsoc, c.omax, part_lpp(c.N, c.nsoc, c.omax, c.oe, /*latency=*/true),
                      (none_cone && !pol.no_ball) ? LF_BALL : 0, c.oe) < 0)
            c = classify(a, b, mode.case4, /*part=*/false);
        if (mode.lat_part && c.status == DCOL_OK && c.oe > 0 && part_lpp(c.N, c.nsoc, c.omax, c.oe, /*latency=*/true) < 2)
            c = classify(a, b, mode.case4, /*part=*/false);
        const SocForm soc = (mode.jac || c.stream) ? SocForm::Dense   // (the streamed kernel's SOC rows are dense)
                            : c.nsoc == 0 ? ((a.boxp && b.boxp && c.N == 4 && c.omax == 12 && c.o == 12 && !pol.no_box)
                                               ? SocForm::Box : SocForm::Dense)
                            : (none_cone && !pol.no_ball) ? SocForm::Ball
                            : (all_cone && c.N == 4 && !pol.no_cone) ? SocForm::Cone : SocForm::Dense;
        // a row-partitioned bucket only where its SOC flavour is compiled: the x polytope
        // (NSOC = 1) buckets exist only with ball rows, so with DCOL_NO_BALL those pairs take
        // the dense-row kernels (N and NSOC do not depend on the partition, so `soc` stands)
        if (c.status == DCOL_OK && c.oe > 0 && !part_flavour_built(c.N, c.nsoc, c.omax, c.oe, c.lpp, soc == SocForm::Ball))
            c = classify(a, b, mode.case4, /*part=*/false);
        // flavour's own list (row-partitioned buckets have theirs: PairClass::lpp)
        if (c.status == DCOL_OK && (soc == SocForm::Ball || soc == SocForm::Cone) && c.oe == 0)
            c.lpp = choose_lpp(c.N, c.nsoc, c.omax, soc == SocForm::Ball ? 2 : 4);
        const BucketKey k = c.status == DCOL_OK ? BucketKey{0, c.N, c.nsoc, c.omax, c.lpp, soc, 0, c.oe, c.stream ? 1 : 0}
                                                : BucketKey{1, 0, 0, 0, 0, SocForm::Dense, c.status, 0, 0};
        auto it = gid_of_key.emplace(k, (int32_t)groups.size()).first;
        if (it->second == (int32_t)groups.size()) groups.push_back(Group{k});
        Group& g = groups[it->second];
        g.full = g.full && c.o == c.omax;
        return it->second;
    };
    // dense cache only when it is small against the batch (its fill is O(S^2): a small
    // batch against a big table takes the hash map)
    const int64_t cells = (int64_t)ns * ns;
    const bool dense = cells <= ((int64_t)1 << 22) && cells <= 16 * B + 4096;
    std::vector<int32_t> cache(dense ? (size_t)ns * ns : 0, -1);
    std::unordered_map<int64_t, int32_t> sparse;
    std::vector<int32_t> gid((size_t)B);
    for (int64_t i = 0; i < B; ++i) {
        const int32_t i1 = s1[i], i2 = s2[i];
        if (i1 < 0 || i1 >= ns || i2 < 0 || i2 >= ns)
            return fail(DCOL_ERR_ARG, "shape id out of range at pair " + std::to_string(i));
        int32_t g;
        if (dense) {
            int32_t& e = cache[(size_t)i1 * ns + i2];
            if (e < 0) e = classify_pair(i1, i2);
            g = e;
        } else {
            auto it = sparse.find((int64_t)i1 * ns + i2);
            if (it == sparse.end()) it = sparse.emplace((int64_t)i1 * ns + i2, classify_pair(i1, i2)).first;
            g = it->second;
        }
        gid[(size_t)i] = g;
        ++groups[g].n;
    }
    // Latency configurations only when the whole plan cannot fill the GPU: the buckets of a
    // large mixed plan run side by side on the fan-out streams, so each keeps its throughput
    // configuration even when it alone would leave SIMDs idle (PlanPolicy::latency_per_launch:
    // the per-launch rule).
    // (the register buckets' lanes: a streamed bucket has one configuration and does not
    // change what the other buckets get -- plan_layout)
    int64_t plan_lanes = 0;
    for (const Group& G : groups)
        if (G.key.kind == 0 && !G.key.stream) plan_lanes += G.n * G.key.lpp;
    p.small = !mode.force_large && plan_lanes < pol.small_lanes(simds);
    p.buckets.clear();
    p.perm.assign((size_t)B, 0);
    int64_t at = 0;
    for (auto& kv : gid_of_key) {   // key order
        Group& G = groups[kv.second];
        G.at = at;
        const bool solve = G.key.kind == 0;
        Bucket L;
        L.kind = G.key.kind;
        L.N = G.key.N;
        L.nsoc = G.key.nsoc;
        L.omax = G.key.omax;
        L.lpp = G.key.lpp;
        L.code = G.key.code;
        L.oe = G.key.oe;
        L.full = solve && G.full;
        L.ball = solve && G.key.soc == SocForm::Ball;
        L.cone = solve && G.key.soc == SocForm::Cone;
        L.box = solve && G.key.soc == SocForm::Box && L.full;
        L.stream = solve && G.key.stream != 0;
        if (L.stream) L.full = false;   // (no padding-free copy: the row count is a run-time value)
        L.slot0 = at;
        L.n = G.n;
        if (solve && !lpp_forced() && L.n * L.lpp < 64LL * simds && (p.small || pol.latency_per_launch))
            latency_config(L);   // cannot fill the GPU
        at += G.n;
        p.buckets.push_back(L);
    }
    for (int64_t i = 0; i < B; ++i) p.perm[(size_t)groups[gid[(size_t)i]].at++] = (int32_t)i;   // stable
    // A streamed bucket's slots in descending row count (stable): its launch is one wave per
    // slot, handed out in slot order as SIMDs free up, so the longest waves start first and
    // the short ones fill the tail -- the packed launch's list-scheduling argument, within a
    // bucket.
    for (Bucket& L : p.buckets) {
        if (!L.stream) continue;
        const auto rows_of = [&](int32_t pi) { return shapes[s1[pi]].n_ort + shapes[s2[pi]].n_ort; };
        const auto first = p.perm.begin() + L.slot0, last = first + L.n;
        std::stable_sort(first, last, [&](int32_t a, int32_t b) { return rows_of(a) > rows_of(b); });
        L.rows = 0;
        for (auto it = first; it != last; ++it) L.rows += (rows_of(*it) + 63) / 64 * 64;
    }
    assign_lanes(p, pol);
    return DCOL_SUCCESS;
}

// One segment per solve bucket with case ids from vid_of (fused_vid / packed_vid), in
// descending per-pair cost (bucket_cost): the workgroup dispatcher hands out blocks in index
// order as SIMDs free up, so the longest-latency waves start first and the short ones fill
// the tail (list scheduling, longest first); PlanPolicy::fused_key_order: key order.  false
// (p unchanged) when a bucket has no case.
inline bool plan_segments(PlanLayout& p, int (*vid_of)(int, int, int, int, int, int), const PlanPolicy& pol) {
    std::vector<int> order;
    for (size_t i = 0; i < p.buckets.size(); ++i)
        if (p.buckets[i].kind == 0 && !p.buckets[i].stream) order.push_back((int)i);
    if (!pol.fused_key_order)
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            const Bucket& A = p.buckets[a];
            const Bucket& B = p.buckets[b];
            return bucket_cost(A) / (double)A.n > bucket_cost(B) / (double)B.n;
        });
    std::vector<FusedSeg> segs;
    int64_t block = 0;
    for (int i : order) {
        const Bucket& L = p.buckets[i];
        const int vid = vid_of(L.N, L.nsoc, L.omax, L.lpp, L.flags(), L.oe);
        if (vid < 0) return false;
        segs.push_back(FusedSeg{vid, L.lpp, block, L.slot0, L.n});
        block += (L.n * L.lpp + kBlock - 1) / kBlock;
    }
    p.segs = std::move(segs);
    p.fused_blocks = block;
    p.packed = false;
    p.lanes = 1;   // no fan-out
    return true;
}

// A plan with a streamed bucket takes the per-bucket launch form, never fused or packed (the
// fused and packed kernels switch over register-kernel cases only).  Its other buckets keep
// their configuration: the policy below looks at the register buckets alone (solve_lanes,
// plan_segments), so they are bucketed and configured exactly as in the plan of the same
// pairs without the streamed ones, and plan_layout then launches every bucket by itself.
inline bool has_stream(const PlanLayout& p) {
    for (const Bucket& L : p.buckets)
        if (L.stream) return true;
    return false;
}

// register solve buckets of a layout and their lanes together (stream: the streamed ones too)
inline std::pair<int, int64_t> solve_lanes(const PlanLayout& p, bool stream = false) {
    int solves = 0;
    int64_t lanes = 0;
    for (const Bucket& L : p.buckets)
        if (L.kind == 0 && (stream || !L.stream)) {
            ++solves;
            lanes += L.n * L.lpp;
        }
    return {solves, lanes};
}

// A plan with several solve buckets that together leave the GPU mostly idle (fewer lanes
// than one wave per SIMD: every bucket already took its latency configuration) runs as ONE
// fused launch; p.segs is left empty when it does not qualify.  Returns 0 when fused, 1 when
// the plan does not qualify (large or single-variant), 2 when it qualifies but a bucket has
// no case in the fused kernel.
inline int plan_fuse(PlanLayout& p, int simds, const PlanPolicy& pol) {
    p.segs.clear();
    p.fused_blocks = 0;
    p.packed = false;
    const auto [solves, lanes] = solve_lanes(p);
    if (solves < 2 || solves > kMaxFusedSegs || lanes >= pol.small_lanes(simds)) return 1;
    return plan_segments(p, fused_vid, pol) ? 0 : 2;
}

// A mid-size plan (not small, below PlanPolicy::pack_lanes) with several solve buckets,
// every one of which the packed kernel has, becomes one packed launch; otherwise p is
// unchanged.
inline void plan_pack(PlanLayout& p, int simds, const PlanPolicy& pol) {
    if (p.small || p.fused()) return;
    const auto [solves, lanes] = solve_lanes(p);
    if (solves < 2 || solves > kMaxFusedSegs || lanes >= pol.pack_limit(simds)) return;
    if (!plan_segments(p, packed_vid, pol)) return;
    p.packed = true;
}

// The layout of the plan of pairs (s1[i], s2[i]), i < B, over `shapes` on a device with
// `simds` SIMDs.  allow_fuse = false (DCOL_PLAN_NO_FUSE): one launch per bucket.  Returns
// DCOL_SUCCESS, or an error with last_error() set.
// case4_stream (DCOL_PLAN_CASE4_STREAM, with case4): BucketMode::case4_stream.
inline int plan_layout(const std::vector<DevShape>& shapes, int simds, int64_t B, const int32_t* s1,
                       const int32_t* s2, bool case4, bool allow_fuse, const PlanPolicy& pol, PlanLayout& out,
                       bool case4_stream = false) {
    BucketMode mode;
    mode.case4 = case4;
    mode.case4_stream = case4 && case4_stream;
    int rc = bucket_pairs(shapes, simds, B, s1, s2, mode, pol, out);
    if (rc != DCOL_SUCCESS) return rc;
    // a plan that cannot fill the GPU: no one-lane row-partitioned buckets (BucketMode::lat_part)
    if (out.small && !lpp_forced())
        for (const Bucket& L : out.buckets) mode.lat_part = mode.lat_part || (L.kind == 0 && L.oe > 0 && L.lpp < 2);
    if (mode.lat_part) {
        rc = bucket_pairs(shapes, simds, B, s1, s2, mode, pol, out);
        if (rc != DCOL_SUCCESS) return rc;
    }
    // only when every bucket the fused kernel lacks is a row-partitioned one (a dense bucket
    // without a case -- a many-row bucket -- keeps the plan unfused whatever the PART pairs
    // do, and they would lose their faster kernels for nothing); when the re-bucketed plan
    // still does not fuse, the first bucketing stands
    bool only_part = true;
    for (const Bucket& L : out.buckets)
        if (L.kind == 0 && L.oe == 0 && !L.stream && fused_vid(L.N, L.nsoc, L.omax, L.lpp, L.flags(), 0) < 0)
            only_part = false;
    if (plan_fuse(out, simds, pol) == 2 && only_part) {
        mode.fused_part = true;
        rc = bucket_pairs(shapes, simds, B, s1, s2, mode, pol, out);
        if (rc != DCOL_SUCCESS) return rc;
        if (plan_fuse(out, simds, pol) == 2) {
            mode.fused_part = false;
            rc = bucket_pairs(shapes, simds, B, s1, s2, mode, pol, out);
            if (rc != DCOL_SUCCESS) return rc;
        }
    }
    if (!allow_fuse && out.fused()) {   // same buckets, launched one by one (fan-out)
        out.segs.clear();
        out.fused_blocks = 0;
        assign_lanes(out, pol);
    }
    if (allow_fuse) plan_pack(out, simds, pol);   // mid-size plans: one packed launch
    // A small plan the fused kernel cannot take (a bucket without a fused case) would fan
    // its latency-configured buckets out over the streams, one under-filled launch after
    // another; the packed launch of its throughput configurations serves it better (one
    // launch, every wave placed as SIMDs free) when every bucket has a
    // packed case.  Tried on a scratch layout: out stands unless it packs.
    if (allow_fuse && out.small && !out.fused() && !lpp_forced() && !pol.small_fanout) {
        BucketMode large;
        large.case4 = case4;
        large.case4_stream = mode.case4_stream;
        large.force_large = true;
        PlanLayout q;
        if (bucket_pairs(shapes, simds, B, s1, s2, large, pol, q) == DCOL_SUCCESS) {
            plan_pack(q, simds, pol);
            if (q.fused()) {
                // q.small is false, and so the pair-server yield sees a large plan: ADVICE.md (kept as is)
                q.issue.clear();
                out = std::move(q);
            }
        }
    }
    // With a streamed bucket: the same buckets, launched one by one over the streams (as under
    // DCOL_PLAN_NO_FUSE); whether the plan can fill the GPU counts the streamed waves too.
    if (has_stream(out)) {
        out.segs.clear();
        out.fused_blocks = 0;
        out.packed = false;
        out.small = solve_lanes(out, /*stream=*/true).second < pol.small_lanes(simds);
        assign_lanes(out, pol);
    }
    return DCOL_SUCCESS;
}

// The layout of a DCOL_PLAN_JACOBIAN plan: the pairs bucketed on the dense-row kernels
// (BucketMode::jac), one launch per bucket over the streams of a plan that fills the GPU --
// never fused or packed, no latency configurations (the Jacobian copies exist at one lane
// count per shape).  stream (DCOL_PLAN_JACOBIAN_STREAM): pairs above the dense-row buckets get
// a streamed bucket per (N, NSOC) as in a plain plan -- slots in descending row count, costed
// by bucket_cost's streamed branch, spread over the streams with the other buckets -- and
// the pairs of at most 128 rows the dense buckets they get without it.
inline int plan_layout_jac(const std::vector<DevShape>& shapes, int simds, int64_t B, const int32_t* s1,
                           const int32_t* s2, bool case4, const PlanPolicy& pol, PlanLayout& out, bool stream = false,
                           bool case4_stream = false) {
    BucketMode mode;
    mode.case4 = case4;
    mode.case4_stream = case4 && case4_stream;   // (streamed only with `stream` too: classify)
    mode.force_large = true;
    mode.jac = true;
    mode.jac_stream = stream;
    const int rc = bucket_pairs(shapes, simds, B, s1, s2, mode, pol, out);
    // (bucketed as a large plan; whether it can fill the GPU still decides if a run asks a
    // resident pair server to leave: the streamed waves count, as in plan_layout)
    if (rc == DCOL_SUCCESS) out.small = solve_lanes(out, /*stream=*/true).second < pol.small_lanes(simds);
    return rc;
}

}  // namespace dcol_host
