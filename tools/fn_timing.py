"""Step time under a per-foot force-bound table (wbc_set_force_bounds) against the limits
instances it extends, on one device in one process: HIP events around back-to-back launches, as bench.py times
a step.

  python tools/fn_timing.py [--steps 2000] [--warmup 50] [--rounds 5] [--passes 2] [--parent-lib PATH]
  python tools/fn_timing.py --oracle-passes 512        (no GPU: the numpy oracle's active-set passes)

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times over:
  plain     no table (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  lm        (-max_torque x 12, +max_torque x 12, friction x 4) in every row (wbc_kernel_lm0.hip): the code the
            force-bound instances extend
  fn        the same limits rows and (-inf x 4, +inf x 4) in every row, the same QPs (wbc_kernel_fn0.hip)
  fn_only   the force-bound default rows without a limits table (wbc_kernel_fn0.hip, a null limits pointer)
  seed7     the same limits rows and tests/force_bounds_oracle.py table(B, 7): other QPs, not the same work
and, with --parent-lib, `parent` and `parent_lm`: the plain step and the limits step of another build of the
library (the parent commit's) on an engine of its own, in the same rotation.  The whole run is repeated `passes`
times; one JSON line per workload and pass with the median us per step of each form, fn over lm (the table's own
cost), seed7 over fn, and this build's plain and lm steps over the parent's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = (("stance_cold", 4096, 1), ("rl_random", 8192, 3))


def oracle_passes(n):
    """Mean active-set passes of the numpy oracle on n robots per workload, no bounds against table(n, 7)."""
    import force_bounds_oracle as FO
    from quadrupedwholebodycontroller_amd import workloads

    for gen, _, seed in WORKLOADS:
        inp = getattr(workloads, gen)(n, seed=seed)
        res = {}
        for name, t in (("default", np.tile(FO.NONE, (n, 1))), ("seed7", FO.table(n))):
            r = FO.run_batch(inp, t)
            res[name] = dict(ok=int((r["status"] == 0).sum()), mean_passes=round(float(r["iters"].mean()), 3),
                             max_passes=int(r["iters"].max()), tight=FO.tight_robots(r["grf"], r["status"], inp["contacts"], t))
        print(json.dumps({"workload": gen, "robots": n, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--oracle-passes", type=int, default=0)
    args = ap.parse_args()
    if args.oracle_passes:
        return oracle_passes(args.oracle_passes)
    import torch

    import force_bounds_oracle as FO
    from quadrupedwholebodycontroller_amd import STATELESS, Engine, _capi, workloads

    stream = torch.cuda.Stream()

    def engine(inp, lib_path=None):
        if lib_path:  # an engine of another build: its own library handle, this build's Python wrapper
            own, _capi._lib = _capi._lib, None
            try:
                _capi.load_library(os.path.abspath(lib_path))
                e = Engine(len(inp["contacts"]))
            finally:
                _capi._lib = own
        else:
            e = Engine(len(inp["contacts"]))
        e.set_stream(stream)
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        return e

    def timed(e):
        for _ in range(args.warmup):
            e.step(STATELESS)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(args.steps):
            e.step(STATELESS)
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / args.steps * 1e3  # us per step

    Engine(4).close()  # this build's library is the process's default before another one is loaded
    for p in range(args.passes):
        for gen, B, seed in WORKLOADS:
            inp = getattr(workloads, gen)(B, seed=seed)
            e = engine(inp)
            parent = engine(inp, args.parent_lib) if args.parent_lib else None
            uniform, none, seed7 = e.limits(), e.force_bounds(), FO.table(B)
            forms = [("plain", None, None), ("lm", uniform, None), ("fn", uniform, none), ("fn_only", None, none),
                     ("seed7", uniform, seed7)]
            us = {name: [] for name, *_ in forms}
            if parent:
                us["parent"], us["parent_lm"] = [], []
            for _ in range(args.rounds):
                for name, lm, fn in forms:
                    e.set_limits(lm)
                    e.set_force_bounds(fn)
                    us[name].append(timed(e))
                if parent:
                    parent.set_limits(None)
                    us["parent"].append(timed(parent))
                    parent.set_limits(uniform)
                    us["parent_lm"].append(timed(parent))
            e.set_limits(None)
            e.set_force_bounds(None)
            e.close()
            if parent:
                parent.set_limits(None)
                parent.close()
            med = {k: float(np.median(v)) for k, v in us.items()}
            print(json.dumps({"pass": p, "workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds,
                              "us_per_step": {k: round(v, 3) for k, v in med.items()},
                              "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
                              "fn_over_lm": round(med["fn"] / med["lm"], 4),
                              "fn_only_over_lm": round(med["fn_only"] / med["lm"], 4),
                              "seed7_over_fn": round(med["seed7"] / med["fn"], 4),
                              "plain_over_parent_plain": round(med["plain"] / med["parent"], 4) if parent else None,
                              "lm_over_parent_lm": round(med["lm"] / med["parent_lm"], 4) if parent else None}), flush=True)


if __name__ == "__main__":
    main()
