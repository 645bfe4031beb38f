"""Step time under a per-robot base-body table (wbc_set_base_body) against the plain step
and the contact-normal instance it extends, on one device in one process: HIP events around back-to-back
launches, as bench.py times a step.

  python tools/bb_timing.py [--steps 200] [--warmup 20] [--rounds 7] [--parent-lib PATH]

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times
over:
  plain     no table (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  flat      normals (0, 0, 1) and the engine's uniform parameter table, the same QPs
            (wbc_kernel_cns.hip / wbc_kernel_cn0.hip): the instance the base-body one extends
  bb        the model's own base in every row, the same QPs (wbc_kernel_bbs.hip / wbc_kernel_bb0.hip)
  bb_dev    the same with the contact masks device-bound, not grouped (wbc_kernel_bb0.hip on both
            workloads: on stance_cold the A/B of the stance-only unit against the any-mask one)
  payload   base_body_oracle.payload_rows(B): other QPs, not the same work
and, with --parent-lib, `parent`: the plain step of another build of the library (the parent commit's)
on an engine of its own, in the same rotation.  Prints one JSON line per workload with the median us
per step of each, the ratios to the plain step, and bb over flat: the table's own increment."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    import torch

    import base_body_oracle as BB
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
        flat = np.array([0.0, 0.0, 1.0])
        default = e.base_body()
        payload = BB.payload_rows(B)
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()
        forms = [("plain", None, None, False), ("flat", flat, None, False), ("bb", None, default, False),
                 ("bb_dev", None, default, True), ("payload", None, payload, False)]
        us = {name: [] for name, *_ in forms}
        if parent:
            us["parent"] = []
        for _ in range(args.rounds):
            for name, n, rows, dev in forms:
                e.set_contact_normals(n)
                e.set_base_body(rows)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                us[name].append(timed(e))
            if parent:
                us["parent"].append(timed(parent))
        e.set_contact_normals(None)
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
                          "bb_over_flat": round(med["bb"] / med["flat"], 4),
                          "bb_dev_over_bb": round(med["bb_dev"] / med["bb"], 4),
                          "bb_over_parent_plain": round(med["bb"] / med["parent"], 4) if parent else None}), flush=True)


if __name__ == "__main__":
    main()
