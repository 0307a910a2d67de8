"""Record what the library's plans launch, over the grid of tests/plan_cases.py:

    python tools/record_plan_layouts.py --commit $(git rev-parse HEAD) [--out tests/plan_layouts.json]

Needs a GPU (plans hold a device table; creating one launches no solve).  One child process
per environment setting -- the policy variables are read once per process -- one after
another, each under its own time limit.  Per plan: table, B, options, environment, the ordered
Plan.buckets() rows (tests/plan_cases.py BUCKET_KEYS), num_launches, num_streams and
launch_form; per file: the commit the library was built from, the device's SIMD count and the
pair seed.  tests/test_plan_layout.py replays the file through the x86 build of the policy,
tests/test_plan_buckets.py through the C-ABI."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "dcol-trajectory-optimization_amd"), REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import plan_cases  # noqa: E402


def child(env, out):
    import torch
    from dcol_amd import spec_from_arrays
    from dcol_amd.engine import Plan, Table
    plans = []
    tables = {}
    for name, B, opts in plan_cases.grid(env):
        if name not in tables:
            tab = plan_cases.table(name)
            tables[name] = Table([spec_from_arrays(tab, k) for k in range(len(tab["type"]))], 0)
        s1, s2 = plan_cases.pairs(name, B)
        p = Plan(tables[name], s1, s2, case4=bool(opts & 1), fuse=not (opts & 2))
        plans.append({"env": env, "table": name, "B": B, "options": opts,
                      "buckets": [plan_cases.bucket_row(b) for b in p.buckets()],
                      "num_launches": p.num_launches, "num_streams": p.num_streams, "launch_form": p.launch_form})
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    with open(out, "w") as f:
        json.dump({"simds": simds, "device": torch.cuda.get_device_name(0), "plans": plans}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "plan_layouts.json"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", nargs=2, metavar=("ENV_JSON", "FILE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(json.loads(a.child[0]), a.child[1])
    rec = {"commit": a.commit, "pair_seed": plan_cases.PAIR_SEED, "plans": []}
    base = {k: v for k, v in os.environ.items() if k not in plan_cases.POLICY_VARS}
    for i, env in enumerate(({},) + plan_cases.ENVS):
        part = f"{a.out}.part{i}"
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
                            "--commit", a.commit, "--child", json.dumps(env), part], env={**base, **env})
        if r.returncode != 0:   # nothing more on the GPU after a failed or timed-out child
            sys.exit(f"child {env} exited with {r.returncode}")
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        for k in ("simds", "device"):
            assert rec.setdefault(k, got[k]) == got[k]
        rec["plans"] += got["plans"]
        print(f"{env or 'default'}: {len(got['plans'])} plans", flush=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rec['plans'])} plans -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
