"""The compiled copies of the solver per launch form, and which of them a plan's bucket launches
(test infrastructure of tests/test_variant_ledger.py and tests/test_variant_parity_gpu.py).

csrc/variants.py is the one list the kernels are generated from; compiled(form) restates, per
launch form, what it generates -- keyed (N, NSOC, OMAX, LPP, FL, OE), with the waves-per-SIMD
request WPS as a seventh field for the per-variant kernels (two SPLIT copies differ in it
alone):

  buckets  one kernel per copy, launched by the per-N launchers.  The order was read from
           csrc/dcol_kernels_n4.hip launch_n4 (lines 18-24: BOX_FD, BOX, FULL_CONE, FULL, BALL,
           CONE, dense; dcol_kernels_n5.hip ... n8.hip lines 18-20 list FULL, BALL, dense, the
           lists the other flavours lack for N > 4), and for a row-partitioned bucket (OE > 0)
           from csrc/dcol_kernels_part.inc part_pass (lines 36-37: SPLIT, then PART) as called
           by dcol_capi.cpp launch_variant (lines 305-315: the (6, 2) ball-row unit before its
           dense-row unit, which keeps a bucket's list order FULL|BALL, BALL, FULL, dense).
           With DCOL_WPS=<w> a first pass takes only copies built for w waves per SIMD.
  fused    the cases of dcol_kernels_fused.hip: fused() + fused_part(), index = case id.
  packed   the cases of dcol_kernels_packed.hip: packed(), index = case id.
  jac      the contact-point Jacobian copies, jac(shapes) (dcol_kernels_jac.hip).
  server   the fused list again: dcol_kernels_server.hip switches over the same cases.

resolve(form, bucket, run_flags) is the launchers' rule: the first listed copy whose FL is a
subset of the bucket's flags plus the run's LF_FDONLY / LF_SPLIT.  For fused and packed it
restates dcol_plan.hpp fused_vid / packed_vid; tests/test_variant_ledger.py pins both to the
case ids the x86 build of the plan policy returns.

Covered elsewhere (not in the ledger): the suspend / resume copies (variants.SUSP,
dcol_kernels_susp.hip) by tests/test_gpu_fullsize.py::test_suspend_resume_bitwise_equal, and
the streamed-row kernels (dcol_kernels_stream.hip, dcol_kernels_stream_jac.hip) by
tests/test_stream_rows_gpu.py::test_stream_* and tests/test_stream_jacobian_gpu.py.
"""
import importlib.util
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
VARIANTS_PY = os.path.join(REPO, "dcol-trajectory-optimization_amd", "csrc", "variants.py")

LF_FULL, LF_BALL, LF_CONE, LF_BOX, LF_SPLIT, LF_FDONLY = 1, 2, 4, 8, 32, 64   # csrc/dcol_launch.hpp
FORMS = ("buckets", "fused", "packed", "jac", "server")
COVERED_ELSEWHERE = {
    "SUSP": "tests/test_gpu_fullsize.py::test_suspend_resume_bitwise_equal",
    "stream": "tests/test_stream_rows_gpu.py::test_stream_*",
    "stream_jac": "tests/test_stream_jacobian_gpu.py::test_stream_*",
}

# wps: 0 for the forms whose cases share one kernel
Copy = namedtuple("Copy", "N nsoc omax lpp fl oe wps")


def load_variants(path=VARIANTS_PY):
    spec = importlib.util.spec_from_file_location("dcol_variants_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def shapes(v):
    return [(n, s, o) for (n, s), os_ in sorted(v.OMAX.items()) for o in os_]


def compiled(form, v=None):
    """The copies of one launch form, in the order its launcher (or case switch) lists them"""
    v = v or load_variants()
    sh = shapes(v)
    if form == "buckets":
        out = [Copy(n, s, o, l, 73, 0, w) for n, s, o, l, w in v.BOX_FD]
        out += [Copy(n, s, o, l, 9, 0, w) for n, s, o, l, w in v.BOX]
        out += [Copy(n, s, o, l, 5, 0, w) for n, s, o in sh if (n, s, o) in v.FULL_CONE for l, w in v.configs_fl(n, s, o, 4)]
        out += [Copy(n, s, o, l, 1, 0, w) for n, s, o in sh if (n, s) in v.FULL for l, w in v.configs(n, s, o)]
        out += [Copy(n, s, o, l, 2, 0, w) for n, s, o in sh if v.ball(n, s) for l, w in v.configs_fl(n, s, o, 2)
                if (n, s, o, l) not in v.BALL_SKIP]
        out += [Copy(n, s, o, l, 4, 0, w) for n, s, o in sh if v.cone(n, s, o) for l, w in v.configs_fl(n, s, o, 4)]
        out += [Copy(n, s, o, l, 0, 0, w) for n, s, o in sh for l, w in v.configs(n, s, o)]
        out += [Copy(n, s, o, l, fl, oe, w) for n, s, o, l, w, fl, oe in v.SPLIT]
        out += [Copy(n, s, o, l, fl, oe, w) for n, s, o, l, w, fl, oe in v.part_variants()]
        return out
    if form in ("fused", "server"):
        return ([Copy(n, s, o, l, fl, 0, 0) for n, s, o, l, fl in v.fused()]
                + [Copy(n, s, o, l, fl, oe, 0) for n, s, o, l, fl, oe in v.fused_part()])
    if form == "packed":
        return [Copy(n, s, o, l, fl, oe, 0) for n, s, o, l, fl, oe in v.packed()]
    if form == "jac":
        return [Copy(n, s, o, l, 0, 0, w) for n, s, o, l, w in v.jac(sh)]
    raise ValueError(form)


_lists = {}


def _list(form):
    if form not in _lists:
        _lists[form] = compiled(form)
    return _lists[form]


def split_built(N, nsoc, omax, oe):
    return any((c.N, c.nsoc, c.omax, c.oe) == (N, nsoc, omax, oe) and c.fl & LF_SPLIT for c in _list("buckets"))


def run_flags(grad, env=None):
    """What a run adds to its buckets' flags: LF_FDONLY without an envelope / implicit gradient,
    LF_SPLIT (checked per bucket in resolve) under DCOL_SPLIT=<non-zero>"""
    env = env or {}
    split = env.get("DCOL_SPLIT")
    return (0 if grad in ("envelope", "implicit") else LF_FDONLY) | (LF_SPLIT if split and int(split) != 0 else 0)


def resolve(form, b, flags=0, wps=0):
    """Index in compiled(form) of the copy that bucket row b (a dict with N, nsoc, omax, lpp, oe,
    flags) launches in a run with run_flags `flags` (and DCOL_WPS=wps), or -1"""
    N, nsoc, omax, lpp, oe, bf = b["N"], b["nsoc"], b["omax"], b["lpp"], b["oe"], b["flags"]
    lst = _list(form)
    same = lambda c: (c.N, c.nsoc, c.omax, c.lpp, c.oe) == (N, nsoc, omax, lpp, oe)  # noqa: E731
    if form == "buckets":
        f = bf | (flags & LF_FDONLY)
        if oe > 0 and lpp == 2 and flags & LF_SPLIT and split_built(N, nsoc, omax, oe):
            f |= LF_SPLIT
        for want_wps in ((wps, 0) if (wps and oe > 0) else (0,)):
            for i, c in enumerate(lst):
                if same(c) and (c.fl & f) == c.fl and (want_wps == 0 or want_wps == c.wps % 10):
                    return i
        return -1
    if form == "jac":
        return next((i for i, c in enumerate(lst) if same(c) and oe == 0), -1)
    if form in ("fused", "server"):   # fused_vid: by flavour in preference order, then the list
        wants = (LF_FULL | LF_BALL, LF_BALL, LF_FULL, 0) if oe > 0 else (LF_FULL, LF_BALL, LF_CONE, 0)
        for want in wants:
            if (want & bf) != want:
                continue
            for i, c in enumerate(lst):
                if same(c) and c.fl == want:
                    return i
        return -1
    if form == "packed":   # packed_vid: the list is in preference order
        return next((i for i, c in enumerate(lst) if same(c) and (c.fl & bf) == c.fl), -1)
    raise ValueError(form)


def _max_lpp(v, N, nsoc, omax, fl):
    """dcol_host.hpp max_lpp: the flavour's largest compiled LPP, the dense kernels' if it has none"""
    has = (fl == 2 and v.ball(N, nsoc) and not any((N, nsoc, omax, l) in v.BALL_SKIP for l, _ in v.configs_fl(N, nsoc, omax, 2))
           ) or (fl == 4 and v.cone(N, nsoc, omax))
    return max(l for l, _ in (v.configs_fl(N, nsoc, omax, fl) if has else v.configs(N, nsoc, omax)))


def latency_bucket(v, N, nsoc, omax, fl):
    """dcol_plan.hpp latency_config of a dense-row bucket: (omax, lpp) it runs at in a small plan"""
    best_o, best_l = omax, _max_lpp(v, N, nsoc, omax, fl)
    for om in v.OMAX[(N, nsoc)]:
        if om <= omax or om > 2 * omax:
            continue
        l = _max_lpp(v, N, nsoc, om, fl)
        if om * best_l < best_o * l:
            best_o, best_l = om, l
    return best_o, best_l


def reachable(sweeps, v=None):
    """{(form, index)} a bucket of classified pairs can launch, whatever the policy: `sweeps` =
    rows of variant_cases.sweep_classes() (with and without the row partition).  A bucket holds
    pairs of one class and one SOC form (every block a ball, every block a cone with N = 4, box
    x box, or dense -- also what DCOL_NO_BALL / NO_CONE / NO_BOX turn the others into); it is
    padding-free when all its pairs fill the rows; it runs at any compiled lanes per pair
    (throughput choice or DCOL_LPP) in its own bucket, or in a small plan at latency_bucket()'s."""
    v = v or load_variants()
    POLYTOPE, CONE = 0, 2
    poss = {}   # (N, nsoc, omax, oe, soc flags) -> {full}
    for _, ta, na, tb, nb, N, nsoc, omax, oe, o in sweeps:
        socs = {0}
        if nsoc == 0:
            if ta == tb == POLYTOPE and na == nb == 6 and N == 4 and omax == 12:
                socs.add(LF_BOX)
        elif CONE not in (ta, tb):
            socs.add(LF_BALL)
        elif all(t in (POLYTOPE, CONE) for t in (ta, tb)) and N == 4:
            socs.add(LF_CONE)
        for soc in socs:
            poss.setdefault((N, nsoc, omax, oe, soc), set()).add(o == omax)
    out = set()
    for (N, nsoc, omax, oe, soc), fills in poss.items():
        rows = []
        flag_sets = {soc | (LF_FULL if True in fills else 0)} | ({soc & ~LF_BOX} if False in fills else set())
        for bf in flag_sets:
            rows += [dict(N=N, nsoc=nsoc, omax=omax, lpp=l, oe=oe, flags=bf) for l in (1, 2, 4, 8, 16)]
        if oe == 0:
            om, l = latency_bucket(v, N, nsoc, omax, soc & (LF_BALL | LF_CONE))
            if om != omax:
                rows.append(dict(N=N, nsoc=nsoc, omax=om, lpp=l, oe=0, flags=soc & ~LF_BOX))
        for b in rows:
            for form in FORMS:
                for rf in ((0, LF_FDONLY, LF_SPLIT, LF_SPLIT | LF_FDONLY) if form == "buckets" else (0,)):
                    for wps in ((0, 1, 2) if form == "buckets" else (0,)):
                        i = resolve(form, b, rf, wps)
                        if i >= 0:
                            out.add((form, i))
    return out


# Copies no case can reach, per form as Copy tuples (N, NSOC, OMAX, LPP, FL, OE, WPS), each with
# why.  tests/test_variant_ledger.py checks the reason of every entry.
#
# UNREACHABLE, reason "classify": no bucket of well-posed pairs launches the copy -- reachable()
# above, over a brute force of emul_lib.classify: every primitive type against every type, 1 to
# 128 faces or 3 to 128 edges, case 4 on and off, with and without the row partition.  This is
# wider than "no pair has the copy's (N, NSOC, OMAX, OE)": for most entries the class exists, and
# it is the copy's flavour (ball rows, padding-free) or lane count that no bucket of the class asks
# for; reachable() models the policy's choices (flag sets, latency buckets, any compiled lane count).
UNREACHABLE = {
    "buckets": [
        (5, 2, 6, 2, 2, 0, 1),   # only cylinder x cone (dense SOC rows) has the class
        (5, 2, 8, 2, 2, 0, 1),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (5, 2, 8, 8, 2, 0, 1),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (6, 2, 2, 2, 2, 0, 1),   # no class: needs a polygon of at most two edges
        (4, 1, 7, 1, 4, 0, 12),   # only cone x 6-face polytope has the class: always padding-free
        (5, 2, 8, 2, 0, 0, 1),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (6, 2, 2, 2, 0, 0, 1),   # no class: needs a polygon of at most two edges
        (7, 2, 4, 4, 0, 0, 1),   # no class: needs a polygon of fewer than three edges
        (8, 2, 4, 4, 0, 0, 1),   # no class: needs a polygon of fewer than three edges
        (5, 2, 2, 2, 2, 2, 1),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 2, 1, 2, 2, 1),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 2, 2, 0, 2, 1),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 2, 1, 0, 2, 1),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 4, 2, 2, 2, 2),   # ball rows only from cylinder x sphere: always padding-free
        (5, 2, 4, 1, 2, 2, 1),   # ball rows only from cylinder x sphere: always padding-free
        (5, 2, 6, 2, 3, 2, 2),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (5, 2, 6, 2, 2, 2, 2),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (5, 2, 6, 2, 1, 2, 2),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 3, 4, 1),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 2, 4, 1),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 1, 4, 1),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 8, 2, 3, 6, 1),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 8, 2, 2, 6, 1),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 8, 2, 1, 6, 1),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
    ],
    "fused": [
        (5, 2, 6, 2, 2, 0, 0),   # only cylinder x cone (dense SOC rows) has the class
        (5, 2, 8, 8, 2, 0, 0),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (6, 2, 2, 2, 0, 0, 0),   # no class: needs a polygon of at most two edges
        (6, 2, 2, 2, 2, 0, 0),   # no class: needs a polygon of at most two edges
        (5, 2, 2, 2, 2, 2, 0),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 4, 2, 2, 2, 0),   # ball rows only from cylinder x sphere: always padding-free
        (5, 2, 6, 2, 3, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (5, 2, 6, 2, 2, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 3, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 2, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
    ],
    "packed": [
        (4, 1, 7, 1, 4, 0, 0),   # only cone x 6-face polytope has the class: always padding-free
        (5, 2, 6, 2, 2, 0, 0),   # only cylinder x cone (dense SOC rows) has the class
        (5, 2, 8, 2, 2, 0, 0),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (5, 2, 8, 2, 0, 0, 0),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (6, 2, 2, 2, 2, 0, 0),   # no class: needs a polygon of at most two edges
        (6, 2, 2, 2, 0, 0, 0),   # no class: needs a polygon of at most two edges
        (5, 2, 2, 2, 2, 2, 0),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 2, 2, 0, 2, 0),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 4, 2, 2, 2, 0),   # ball rows only from cylinder x sphere: always padding-free
        (5, 2, 6, 2, 3, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (5, 2, 6, 2, 2, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (5, 2, 6, 2, 1, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 3, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 2, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 1, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 8, 2, 3, 6, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 8, 2, 2, 6, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 8, 2, 1, 6, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
    ],
    "jac": [
        (5, 2, 8, 2, 0, 0, 1),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (6, 2, 2, 2, 0, 0, 1),   # no class: needs a polygon of at most two edges
        (7, 2, 4, 4, 0, 0, 1),   # no class: needs a polygon of fewer than three edges
        (8, 2, 4, 4, 0, 0, 1),   # no class: needs a polygon of fewer than three edges
    ],
    "server": [
        (5, 2, 6, 2, 2, 0, 0),   # only cylinder x cone (dense SOC rows) has the class
        (5, 2, 8, 8, 2, 0, 0),   # no class; only cylinder x cone's latency bucket (dense SOC rows, 8 lanes) lands here
        (6, 2, 2, 2, 0, 0, 0),   # no class: needs a polygon of at most two edges
        (6, 2, 2, 2, 2, 0, 0),   # no class: needs a polygon of at most two edges
        (5, 2, 2, 2, 2, 2, 0),   # only capsule x sphere has the class: always padding-free ball rows
        (5, 2, 4, 2, 2, 2, 0),   # ball rows only from cylinder x sphere: always padding-free
        (5, 2, 6, 2, 3, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (5, 2, 6, 2, 2, 2, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 3, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
        (6, 2, 6, 2, 2, 4, 0),   # only a cone partner has the class, with a row to spare: dense SOC rows, padded
    ],
}

# UNREACHABLE_ORACLE, reason "oracle": every copy of (4, 0, 4).  Its pairs are polytope pairs of at
# most four faces together, all unbounded shapes.  With fewer than four faces (half-space x
# half-space, half-space x slab: the padded copies' pairs) no pose has a proper optimum: the C
# oracle fails or returns the degenerate alpha = 0.  With exactly four (slab x slab, half-space x
# wedge) the problem has four rows in four unknowns: the least-squares starting point of the PDIP
# (oracle/dcol_oracle.c pdip, dcol_device.hpp initialize) solves G x = h exactly, the starting
# slack s = G x - h is rounding noise, and bring2cone lifts it to ~1 only if one of its four
# entries is <= 0.  When all four happen to round above zero, mu = s'z / deg is ~1e-17 < tol and
# the solve returns after 0 iterations -- with the right alpha: x is the one vertex -- else after
# 3.  The reference's iteration count is a coin of rounding signs, so no pose gives a reference
# for the count (measured: one pair of 67 returned after 0 iterations on the device and after 3 in
# the oracle, alpha equal to 2e-15), and the class has no case.
UNREACHABLE_ORACLE = {
    "buckets": [(4, 0, 4, 2, 1, 0, 1), (4, 0, 4, 2, 0, 0, 1)],
    "fused": [(4, 0, 4, 2, 0, 0, 0), (4, 0, 4, 2, 1, 0, 0)],
    "packed": [(4, 0, 4, 2, 1, 0, 0), (4, 0, 4, 2, 0, 0, 0)],
    "jac": [(4, 0, 4, 2, 0, 0, 1)],
    "server": [(4, 0, 4, 2, 0, 0, 0), (4, 0, 4, 2, 1, 0, 0)],
}


def unreachable(reason=None):
    """{(form, index in compiled(form))} of the entries with the reason (None: all)"""
    out = set()
    for why, table in (("classify", UNREACHABLE), ("oracle", UNREACHABLE_ORACLE)):
        if reason in (None, why):
            for form, keys in table.items():
                lst = [tuple(c) for c in _list(form)]
                out |= {(form, lst.index(k)) for k in keys}
    return out
