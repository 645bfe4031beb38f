"""Step time under per-robot contact normals (wbc_set_contact_normals) against the plain
step, on one device in one process: HIP events around back-to-back launches, as bench.py times a step.

  python tools/cn_timing.py [--steps 200] [--warmup 20] [--rounds 7] [--parent-lib PATH]

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times
over:
  plain     no table (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  uniform   a uniform parameter table, the same QPs (wbc_kernel_rps.hip / wbc_kernel_rp0.hip)
  flat      normals (0, 0, 1), the same QPs (wbc_kernel_cns.hip / wbc_kernel_cn0.hip)
  flat_dev  the same with the contact masks device-bound, not grouped (wbc_kernel_cn0.hip on both
            workloads: on stance_cold the A/B of the stance-only unit against the any-mask one)
  sloped    contact_normals_oracle.normals(B, 5, 0.35): other QPs (see --passes)
and, with --parent-lib, `parent`: the plain step of another build of the library (the parent commit's)
on an engine of its own, in the same rotation.  Prints one JSON line per workload with the median us
per step of each and the ratios to the plain step.

  python tools/cn_timing.py --passes [--batch 512]
no device: the numpy oracle's reduced active-set pass count (iters) per QP on flat and on sloped
ground over the first `batch` robots of each workload, so that harder QPs are not read as a slower
kernel."""
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


def passes(batch):
    import contact_normals_oracle as CN
    from quadrupedwholebodycontroller_amd import workloads

    for gen, _, seed in WORKLOADS:
        inp = getattr(workloads, gen)(batch, seed=seed)
        nrm = CN.normals(batch, 5, 0.35)
        it = {"flat": [], "sloped": []}
        for b in range(batch):
            for name, n in (("flat", CN.FLAT), ("sloped", nrm[b])):
                r = CN.reduced_step(CN.controller(inp, b, n))
                if r is not None and r[2] == 0:
                    it[name].append(r[3])
        print(json.dumps({"workload": gen, "batch": batch, "mean_passes": {k: round(float(np.mean(v)), 3) for k, v in it.items()},
                          "max_passes": {k: int(np.max(v)) for k, v in it.items()}, "solved": {k: len(v) for k, v in it.items()}}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    if args.passes:
        return passes(args.batch)
    import torch

    import contact_normals_oracle as CN
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
        uniform = e.robot_params()
        flat = np.array([0.0, 0.0, 1.0])
        sloped = CN.normals(B, 5, 0.35)
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()
        forms = [("plain", None, None, False), ("uniform", uniform, None, False), ("flat", None, flat, False),
                 ("flat_dev", None, flat, True), ("sloped", None, sloped, False)]
        us = {name: [] for name, *_ in forms}
        if parent:
            us["parent"] = []
        for _ in range(args.rounds):
            for name, t, n, dev in forms:
                e.set_robot_params(t)
                e.set_contact_normals(n)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                us[name].append(timed(e))
            if parent:
                us["parent"].append(timed(parent))
        e.set_robot_params(None)
        e.set_contact_normals(None)
        e.bind_device_inputs()
        e.close()
        if parent:
            parent.close()
        med = {k: float(np.median(v)) for k, v in us.items()}
        base = med["parent"] if parent else med["plain"]
        print(json.dumps({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds,
                          "us_per_step": {k: round(v, 3) for k, v in med.items()},
                          "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()},
                          "over_plain": {k: round(v / med["plain"], 4) for k, v in med.items()},
                          "flat_over_parent_plain": round(med["flat"] / base, 4) if parent else None}), flush=True)


if __name__ == "__main__":
    main()
