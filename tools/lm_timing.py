"""Step time under a per-robot limits table (wbc_set_limits) against the plain step and the
base-body instances it extends, on one device in one process: HIP events around back-to-back launches, as
bench.py times a step.

  python tools/lm_timing.py [--steps 2000] [--warmup 50] [--rounds 5] [--parent-lib PATH]
  python tools/lm_timing.py --oracle-passes 512        (no GPU: the numpy oracle's active-set passes)

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times over:
  plain     no table (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  bb        the model's own base in every row, with the engine's flat normals and uniform parameters, the same
            QPs (wbc_kernel_bbs.hip / wbc_kernel_bb0.hip): the code the limits instances extend
  bb_dev    the same with the contact masks device-bound, not grouped (wbc_kernel_bb0.hip on both workloads:
            lm0 has no stance-only form, so on stance_cold this is its like-for-like base)
  lm        (-max_torque x 12, +max_torque x 12, friction x 4) in every row, the same QPs (wbc_kernel_lm0.hip)
  seed7     tests/limits_oracle.py table(B, 7): other QPs, not the same work
and, with --parent-lib, `parent`: the plain step of another build of the library (the parent commit's) on an
engine of its own, in the same rotation.  Prints one JSON line per workload with the median us per step of
each, the ratios to the plain step, and lm over bb: the table's own cost."""
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
    """Mean active-set passes of the numpy oracle on n robots per workload, default rows against table(n, 7)."""
    import limits_oracle as LO
    from quadrupedwholebodycontroller_amd import workloads

    for gen, _, seed in WORKLOADS:
        inp = getattr(workloads, gen)(n, seed=seed)
        res = {}
        for name, t in (("default", np.tile(LO.default_row(), (n, 1))), ("seed7", LO.table(n))):
            r = LO.run_batch(inp, t)
            res[name] = dict(ok=int((r["status"] == 0).sum()), mean_passes=round(float(r["iters"].mean()), 3),
                             max_passes=int(r["iters"].max()), tight=LO.tight_torque_robots(r, t))
        print(json.dumps({"workload": gen, "robots": n, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--oracle-passes", type=int, default=0)
    args = ap.parse_args()
    if args.oracle_passes:
        return oracle_passes(args.oracle_passes)
    import torch

    import limits_oracle as LO
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
    for gen, B, seed in WORKLOADS:
        inp = getattr(workloads, gen)(B, seed=seed)
        e = engine(inp)
        parent = engine(inp, args.parent_lib) if args.parent_lib else None
        base, uniform, seed7 = e.base_body(), e.limits(), LO.table(B)
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()
        forms = [("plain", None, None, False), ("bb", base, None, False), ("bb_dev", base, None, True),
                 ("lm", None, uniform, False), ("seed7", None, seed7, False)]
        us = {name: [] for name, *_ in forms}
        if parent:
            us["parent"] = []
        for _ in range(args.rounds):
            for name, rows, lm, dev in forms:
                e.set_base_body(rows)
                e.set_limits(lm)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                us[name].append(timed(e))
            if parent:
                us["parent"].append(timed(parent))
        e.set_base_body(None)
        e.set_limits(None)
        e.bind_device_inputs()
        e.close()
        if parent:
            parent.close()
        med = {k: float(np.median(v)) for k, v in us.items()}
        print(json.dumps({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds,
                          "us_per_step": {k: round(v, 3) for k, v in med.items()},
                          "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
                          "over_plain": {k: round(v / med["plain"], 4) for k, v in med.items()},
                          "lm_over_bb": round(med["lm"] / med["bb"], 4),
                          "lm_over_bb_dev": round(med["lm"] / med["bb_dev"], 4),
                          "seed7_over_lm": round(med["seed7"] / med["lm"], 4),
                          "plain_over_parent_plain": round(med["plain"] / med["parent"], 4) if parent else None}), flush=True)


if __name__ == "__main__":
    main()
