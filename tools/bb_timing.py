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

import numpy as np

import step_timing_common as T


def main():
    ap = argparse.ArgumentParser()
    T.add_timing_arguments(ap, steps=200, warmup=20, rounds=7)
    args = ap.parse_args()
    import torch

    import base_body_oracle as BB
    from quadrupedwholebodycontroller_amd import STATELESS, workloads

    stream = torch.cuda.Stream()
    T.first_engine()
    for gen, B, seed in T.WORKLOADS:
        inp = getattr(workloads, gen)(B, seed=seed)
        e = T.engine(inp, None, stream)
        parent = T.engine(inp, args.parent_lib, stream) if args.parent_lib else None
        flat = np.array([0.0, 0.0, 1.0])
        default = e.base_body()
        payload = BB.payload_rows(B)
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()

        def form(n, rows, dev):
            def measure():
                e.set_contact_normals(n)
                e.set_base_body(rows)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                return T.timed(e, args.steps, args.warmup, stream, STATELESS)
            return measure

        forms = [("plain", form(None, None, False)), ("flat", form(flat, None, False)), ("bb", form(None, default, False)),
                 ("bb_dev", form(None, default, True)), ("payload", form(None, payload, False))]
        if parent:
            forms.append(("parent", lambda: T.timed(parent, args.steps, args.warmup, stream, STATELESS)))
        us = T.rotate(args.rounds, forms)
        e.set_contact_normals(None)
        e.set_base_body(None)
        e.bind_device_inputs()
        e.close()
        if parent:
            parent.close()
        T.report({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds}, us,
                 lambda m: {"bb_over_flat": T.ratio(m, "bb", "flat"), "bb_dev_over_bb": T.ratio(m, "bb_dev", "bb"),
                            "bb_over_parent_plain": T.ratio(m, "bb", "parent")})


if __name__ == "__main__":
    main()
