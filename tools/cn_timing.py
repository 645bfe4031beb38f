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

import numpy as np

import step_timing_common as T


def passes(batch):
    import contact_normals_oracle as CN
    from quadrupedwholebodycontroller_amd import workloads

    for gen, _, seed in T.WORKLOADS:
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
    T.add_timing_arguments(ap, steps=200, warmup=20, rounds=7)
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    if args.passes:
        return passes(args.batch)
    import torch

    import contact_normals_oracle as CN
    from quadrupedwholebodycontroller_amd import STATELESS, workloads

    stream = torch.cuda.Stream()
    T.first_engine()
    for gen, B, seed in T.WORKLOADS:
        inp = getattr(workloads, gen)(B, seed=seed)
        e = T.engine(inp, None, stream)
        parent = T.engine(inp, args.parent_lib, stream) if args.parent_lib else None
        uniform = e.robot_params()
        flat = np.array([0.0, 0.0, 1.0])
        sloped = CN.normals(B, 5, 0.35)
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()

        def form(t, n, dev):
            def measure():
                e.set_robot_params(t)
                e.set_contact_normals(n)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                return T.timed(e, args.steps, args.warmup, stream, STATELESS)
            return measure

        forms = [("plain", form(None, None, False)), ("uniform", form(uniform, None, False)), ("flat", form(None, flat, False)),
                 ("flat_dev", form(None, flat, True)), ("sloped", form(None, sloped, False))]
        if parent:
            forms.append(("parent", lambda: T.timed(parent, args.steps, args.warmup, stream, STATELESS)))
        us = T.rotate(args.rounds, forms)
        e.set_robot_params(None)
        e.set_contact_normals(None)
        e.bind_device_inputs()
        e.close()
        if parent:
            parent.close()
        T.report({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds}, us,
                 lambda m: {"flat_over_parent_plain": T.ratio(m, "flat", "parent")})


if __name__ == "__main__":
    main()
