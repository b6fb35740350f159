#!/usr/bin/env python3
"""Writes tests/golden/capi_plan_parent/plan.json: the table of tests/test_gpu_capi_plan.py (its TABLE and
run_row) run against a build of the commit BEFORE the kernel plan and the split of ppo_capi.hip. Run once, on
an MI355X, never against the code under test:

    PPO_HIP_LIB=<parent checkout>/ppo.cpp_amd/lib/libppo_hip.so python scripts/record_capi_parent.py [OUT.json]

The parent's ppo_amd package is not needed: the binding did not change, only the library it loads."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ppo.cpp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    if not os.environ.get("PPO_HIP_LIB"):
        sys.exit("PPO_HIP_LIB must name the parent commit's libppo_hip.so")
    import test_gpu_capi_plan as T

    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for r in T.TABLE:
        rec[r["name"]] = T.run_row(r)
        print(r["name"], rec[r["name"]].get("error") or rec[r["name"]]["kernel_info"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} rows -> {out}")


if __name__ == "__main__":
    main()
