"""Step time of wbc_step_modes with the objective and the best-mode selection (WBC_OBJECTIVE / WBC_BEST,
DESIGN.md 19) against the step without them, on one device in one process: HIP events around back-to-back
steps, as bench.py times a step.

  python tools/modes_obj_timing.py [--steps 200] [--warmup 20] [--rounds 7] [--parent-lib PATH]

The workload is BASELINE configs[4]'s shard (workloads.mode_states(1024, 4): 1024 states x 16 masks,
B = 16 384).  One engine runs, in turn and `rounds` times over, each step with WBC_STATELESS | WBC_NO_X as
bench.py steps it:
  plain      no flag: the mode loop (wbc_kernel_modes.hip), the parent commit's kernel
  objective  WBC_OBJECTIVE: the loop's objective instance (wbc_kernel_modes_obj.hip)
  best       WBC_BEST: the same, then wbc_best_mode_kernel, a second dependent launch
  plain_x, objective_x   the first two without WBC_NO_X: the objective needs the x the step otherwise skips
             under WBC_NO_X (a, qdd, s), so objective over plain_x is the objective's own sum and store
and, with --parent-lib, `parent`: the plain step of another build of the library (the parent commit's) on
an engine of its own, in the same rotation.  Prints one JSON line with the median us per step of each, the
min and max over the rounds, and the ratios to the plain step."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--states", type=int, default=1024)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import torch

    from quadrupedwholebodycontroller_amd import BEST, NO_X, OBJECTIVE, STATELESS, Engine, _capi, workloads

    stream = torch.cuda.Stream()
    inp, modes = workloads.mode_states(args.states, 4)
    B = args.states * len(modes)

    def engine(lib_path=None):
        if lib_path:  # an engine of another build: its own library handle, this build's Python wrapper
            own, _capi._lib = _capi._lib, None
            try:
                _capi.load_library(os.path.abspath(lib_path))
                e = Engine(B)
            finally:
                _capi._lib = own
        else:
            e = Engine(B)
        e.set_stream(stream)
        e.set_modes(modes)
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        return e

    def timed(e, flags):
        for _ in range(args.warmup):
            e.step_modes(flags)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        for _ in range(args.steps):
            e.step_modes(flags)
        ev1.record(stream)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / args.steps * 1e3  # us per step

    Engine(4).close()  # this build's library is the process's default before another one is loaded
    e = engine()
    parent = engine(args.parent_lib) if args.parent_lib else None
    base = STATELESS | NO_X
    forms = [("plain", base), ("objective", base | OBJECTIVE), ("best", base | BEST), ("plain_x", STATELESS),
             ("objective_x", STATELESS | OBJECTIVE)]
    us = {name: [] for name, _ in forms}
    if parent:
        us["parent"] = []
    for _ in range(args.rounds):
        if parent:
            us["parent"].append(timed(parent, base))
        for name, flags in forms:
            us[name].append(timed(e, flags))
    m = e.modes_per_wave()
    e.close()
    if parent:
        parent.close()
    med = {k: float(np.median(v)) for k, v in us.items()}
    print(json.dumps({"workload": "mode_states", "states": args.states, "modes": len(modes), "batch": B, "modes_per_wave": m,
                      "steps": args.steps, "rounds": args.rounds,
                      "us_per_step": {k: round(v, 3) for k, v in med.items()},
                      "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
                      "over_plain": {k: round(v / med["plain"], 4) for k, v in med.items()},
                      "best_minus_objective_us": round(med["best"] - med["objective"], 3),
                      "objective_over_plain_x": round(med["objective"] / med["plain_x"], 4),
                      "objective_x_over_plain_x": round(med["objective_x"] / med["plain_x"], 4)}), flush=True)


if __name__ == "__main__":
    main()
