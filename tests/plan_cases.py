"""The grid of plans whose layout tests/plan_layouts.json records (test infrastructure, shared
by tools/record_plan_layouts.py, tests/test_plan_layout.py and tests/test_plan_buckets.py).

Tables: the benchmark's prisms, its mixed table, and the stress table (many-faced polytopes
and polygons: the buckets above the fused / packed kernels' row limit, the PART misfits).
Sizes on both sides of the small-plan (64 x SIMDs lanes) and packed-plan (16 x 64 x SIMDs)
thresholds.  Every plan-option combination under the default environment; each policy
variable alone on the mixed table."""
import numpy as np

TABLES = ("prisms", "mixed", "random")
SIZES = (0, 1, 2, 200, 2_000, 31_250, 150_000, 1_000_000)
OPTIONS = (0, 1, 2, 3)            # DCOL_PLAN_CASE4 = 1, DCOL_PLAN_NO_FUSE = 2
PAIR_SEED = 3
ENV_SIZES = (2_000, 150_000, 1_000_000)
ENVS = ({"DCOL_NO_BALL": "1"}, {"DCOL_NO_BOX": "1"}, {"DCOL_NO_CONE": "1"}, {"DCOL_NO_PART": "1"},
        {"DCOL_SMALL_FANOUT": "1"}, {"DCOL_PACK_LANES": "0"}, {"DCOL_NO_FANOUT": "1"},
        {"DCOL_LATENCY_PER_LAUNCH": "1"}, {"DCOL_SIDE_STREAMS": "1"})
# every variable the plan policy reads (a caller's setting of one changes the layouts)
POLICY_VARS = ("DCOL_NO_BALL", "DCOL_NO_BOX", "DCOL_NO_CONE", "DCOL_NO_PART", "DCOL_SMALL_PLAN_LANES",
               "DCOL_PACK_LANES", "DCOL_SMALL_FANOUT", "DCOL_LATENCY_PER_LAUNCH", "DCOL_NO_FANOUT",
               "DCOL_FUSED_ORDER", "DCOL_SIDE_STREAMS", "DCOL_SIDE_STREAMS_LARGE", "DCOL_LPP", "DCOL_SPLIT")
BUCKET_KEYS = ("kind", "N", "nsoc", "omax", "lpp", "oe", "flags", "status", "pairs")

_tables, _pairs = {}, {}


def table(name):
    if name not in _tables:
        import bench
        import stress_shapes
        _tables[name] = {"prisms": lambda: bench.shape_table(64, 0), "mixed": bench.mixed_table,
                         "random": lambda: stress_shapes.random_table(np.random.default_rng(0))}[name]()
    return _tables[name]


def pairs(name, B, seed=PAIR_SEED):
    """(s1, s2) of the B-pair batch on a table: the benchmarks' own generators; uniform shape
    ids on the stress table"""
    if (name, B, seed) not in _pairs:
        import bench
        tab = table(name)
        if name == "prisms":
            s = bench.pairs(B, 64, seed)[:2]
        elif name == "mixed":
            s = bench.mixed_pairs(tab, B, seed)[:2]
        else:
            rng = np.random.default_rng(seed)
            S = len(tab["type"])
            s = rng.integers(0, S, B).astype(np.int32), rng.integers(0, S, B).astype(np.int32)
        _pairs[(name, B, seed)] = s
    return _pairs[(name, B, seed)]


def grid(env):
    """(table, B, options) of the plans recorded under one environment setting"""
    if not env:
        return [(t, B, o) for t in TABLES for B in SIZES for o in OPTIONS]
    return [("mixed", B, 0) for B in ENV_SIZES]


def bucket_row(b):
    """a Plan.buckets() dict as the record's row of ints (kind 0 solve, 1 reject)"""
    return [0 if b["kind"] == "solve" else 1] + [int(b[k]) for k in BUCKET_KEYS[1:]]
