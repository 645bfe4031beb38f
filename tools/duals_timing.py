"""Step time with the QP multipliers written (wbc_step with WBC_DUALS) against the plain step
and the default-row base-body instance the duals units extend, on one device in one process: HIP events
around back-to-back launches, as bench.py times a step.

  python tools/duals_timing.py [--steps 200] [--warmup 20] [--rounds 7] [--parent-lib PATH]

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times over:
  plain     no table, no flag (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  bb        the model's own base in every row, the same QPs (wbc_kernel_bbs.hip / wbc_kernel_bb0.hip)
  duals     no table, WBC_DUALS (wbc_kernel_du0.hip on both workloads: the bb configuration with the
            multipliers' 24 shuffles and three stores per lane)
  bb_dev, duals_dev   the same two with the contact masks device-bound, not grouped: wbc_kernel_bb0.hip
            against wbc_kernel_du0.hip on both workloads (on stance_cold `bb` is the stance-only unit, which
            the duals have no counterpart of, so this pair is the flag's own cost there)
and, with --parent-lib, `parent`: the plain step of another build of the library (the parent commit's) on
an engine of its own, in the same rotation.  Prints one JSON line per workload with the median us per
step of each, the ratios to the plain step, and duals over bb (host-copied and device-bound masks)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("stance_cold", 4096, 1), ("rl_random", 8192, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import torch

    from quadrupedwholebodycontroller_amd import DUALS, STATELESS, Engine, _capi, workloads

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

    def timed(e, flags):
        for _ in range(args.warmup):
            e.step(flags)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(args.steps):
            e.step(flags)
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / args.steps * 1e3  # us per step

    Engine(4).close()  # this build's library is the process's default before another one is loaded
    for gen, B, seed in WORKLOADS:
        inp = getattr(workloads, gen)(B, seed=seed)
        e = engine(inp)
        parent = engine(inp, args.parent_lib) if args.parent_lib else None
        default = e.base_body()
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()
        forms = [("plain", None, STATELESS, False), ("bb", default, STATELESS, False), ("duals", None, STATELESS | DUALS, False),
                 ("bb_dev", default, STATELESS, True), ("duals_dev", None, STATELESS | DUALS, True)]
        us = {name: [] for name, *_ in forms}
        if parent:
            us["parent"] = []
        for _ in range(args.rounds):
            for name, rows, flags, dev in forms:
                e.set_base_body(rows)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                us[name].append(timed(e, flags))
            if parent:
                us["parent"].append(timed(parent, STATELESS))
        e.set_base_body(None)
        e.bind_device_inputs()
        e.close()
        if parent:
            parent.close()
        med = {k: float(np.median(v)) for k, v in us.items()}
        print(json.dumps({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds,
                          "us_per_step": {k: round(v, 3) for k, v in med.items()},
                          "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
                          "over_plain": {k: round(v / med["plain"], 4) for k, v in med.items()},
                          "duals_over_bb": round(med["duals"] / med["bb"], 4),
                          "duals_dev_over_bb_dev": round(med["duals_dev"] / med["bb_dev"], 4),
                          "plain_over_parent": round(med["plain"] / med["parent"], 4) if parent else None}), flush=True)


if __name__ == "__main__":
    main()
