"""Step time under a per-robot parameter table (wbc_set_robot_params) against the plain
step, on one device in one process: HIP events around back-to-back launches, as bench.py times a step.

  python tools/rp_timing.py [--steps 200] [--warmup 20] [--rounds 7]

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times
over, the plain step (engine-wide wbc_params: wbc_kernel_stance.hip / wbc_kernel_step0.hip), the step
under a uniform table (every row the engine-wide values, so the same QPs: wbc_kernel_rps.hip /
wbc_kernel_rp0.hip) and under a heterogeneous one (numpy rng(7) over the tests' ranges).  Prints one
JSON line per workload with the median us per step of each and the ratios to the plain step.
WBC_LIB selects another build of the library (e.g. `make ab NAME=nostance DEFS=-DWBC_NO_STANCE_TU`,
whose engine never picks the stance-only units)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RANGES = dict(friction=(0.35, 1.5), max_torque=(15, 80), kp=(3000, 9000), kp_z=(5000, 15000), kd=(900, 2700), ki=(0, 50),
              kp_swing=(125, 500), kd_swing=(10, 40), slack_weight=(100, 10000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from quadrupedwholebodycontroller_amd import ROBOT_PARAM_NAMES, STATELESS, Engine, workloads

    stream = torch.cuda.Stream()

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

    for gen, B, seed in (("stance_cold", 4096, 1), ("rl_random", 8192, 3)):
        inp = getattr(workloads, gen)(B, seed=seed)
        e = Engine(B)
        e.set_stream(stream)
        e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
        e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
        uniform = e.robot_params()
        g = np.random.default_rng(7)
        mixed = np.zeros((B, 10))
        for c, name in enumerate(ROBOT_PARAM_NAMES):
            mixed[:, c] = g.uniform(*RANGES[name], B)
        us = {"plain": [], "uniform": [], "mixed": []}
        for _ in range(args.rounds):
            for name, t in (("plain", None), ("uniform", uniform), ("mixed", mixed)):
                e.set_robot_params(t)
                us[name].append(timed(e))
        e.set_robot_params(None)
        e.close()
        med = {k: float(np.median(v)) for k, v in us.items()}
        print(json.dumps({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds,
                          "us_per_step": {k: round(v, 3) for k, v in med.items()},
                          "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
                          "uniform_over_plain": round(med["uniform"] / med["plain"], 4),
                          "mixed_over_plain": round(med["mixed"] / med["plain"], 4)}), flush=True)


if __name__ == "__main__":
    main()
