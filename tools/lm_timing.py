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

import numpy as np

import step_timing_common as T


def oracle_passes(n):
    """Mean active-set passes of the numpy oracle on n robots per workload, default rows against table(n, 7)."""
    import limits_oracle as LO

    T.oracle_passes(n, lambda n: (("default", np.tile(LO.default_row(), (n, 1))), ("seed7", LO.table(n))), LO.run_batch,
                    lambda r, t, inp: LO.tight_torque_robots(r, t))


def main():
    ap = argparse.ArgumentParser()
    T.add_timing_arguments(ap, steps=2000, warmup=50, rounds=5)
    ap.add_argument("--oracle-passes", type=int, default=0)
    args = ap.parse_args()
    if args.oracle_passes:
        return oracle_passes(args.oracle_passes)
    import torch

    import limits_oracle as LO
    from quadrupedwholebodycontroller_amd import STATELESS, workloads

    stream = torch.cuda.Stream()
    T.first_engine()
    for gen, B, seed in T.WORKLOADS:
        inp = getattr(workloads, gen)(B, seed=seed)
        e = T.engine(inp, None, stream)
        parent = T.engine(inp, args.parent_lib, stream) if args.parent_lib else None
        base, uniform, seed7 = e.base_body(), e.limits(), LO.table(B)
        masks = torch.from_numpy(inp["contacts"]).cuda()
        torch.cuda.synchronize()

        def form(rows, lm, dev):
            def measure():
                e.set_base_body(rows)
                e.set_limits(lm)
                e.bind_device_inputs(contacts=masks.data_ptr() if dev else 0)
                return T.timed(e, args.steps, args.warmup, stream, STATELESS)
            return measure

        forms = [("plain", form(None, None, False)), ("bb", form(base, None, False)), ("bb_dev", form(base, None, True)),
                 ("lm", form(None, uniform, False)), ("seed7", form(None, seed7, False))]
        if parent:
            forms.append(("parent", lambda: T.timed(parent, args.steps, args.warmup, stream, STATELESS)))
        us = T.rotate(args.rounds, forms)
        e.set_base_body(None)
        e.set_limits(None)
        e.bind_device_inputs()
        e.close()
        if parent:
            parent.close()
        T.report({"workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds}, us,
                 lambda m: {"lm_over_bb": T.ratio(m, "lm", "bb"), "lm_over_bb_dev": T.ratio(m, "lm", "bb_dev"),
                            "seed7_over_lm": T.ratio(m, "seed7", "lm"), "plain_over_parent_plain": T.ratio(m, "plain", "parent")})


if __name__ == "__main__":
    main()
