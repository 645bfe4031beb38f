"""Step time under a per-robot force-task table (wbc_set_force_task) against the force-bound
instances it extends, on one device in one process: HIP events around back-to-back launches, as bench.py times
a step.

  python tools/ft_timing.py [--steps 2000] [--warmup 50] [--rounds 5] [--passes 2] [--parent-lib PATH]
  python tools/ft_timing.py --oracle-passes 512        (no GPU: the numpy oracle's active-set passes)

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times over:
  plain     no table (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  fn        (-inf x 4, +inf x 4) in every row and no other table (wbc_kernel_fn0.hip): the code the force-task
            instances extend
  ft        the same force-bound rows and (0 x 12, 1, 0) in every row, the same QPs (wbc_kernel_ft0.hip)
  ft_only   the force-task default rows alone (wbc_kernel_ft0.hip, the engine's own no-bounds table)
  seed11    tests/force_task_oracle.py table(B, 11, contacts) alone: other QPs, not the same work
and, with --parent-lib, `parent` and `parent_fn`: the plain step and the force-bound step of another build of the
library (the parent commit's) on an engine of its own, in the same rotation.  The whole run is repeated `passes`
times; one JSON line per workload and pass with the median us per step of each form, ft over fn (the table's own
cost), seed11 over ft, and this build's plain and fn steps over the parent's."""
import argparse

import numpy as np

import step_timing_common as T


def oracle_passes(n):
    """Mean active-set passes of the numpy oracle on n robots per workload, the plain rows against table(n, 11)."""
    import force_task_oracle as FT

    T.oracle_passes(n, lambda n: (("default", np.tile(FT.PLAIN, (n, 1))), ("seed11", FT.table(n))), FT.run_batch,
                    lambda r, t, inp: None)


def main():
    ap = argparse.ArgumentParser()
    T.add_timing_arguments(ap, steps=2000, warmup=50, rounds=5)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--oracle-passes", type=int, default=0)
    args = ap.parse_args()
    if args.oracle_passes:
        return oracle_passes(args.oracle_passes)
    import torch

    import force_task_oracle as FT
    from quadrupedwholebodycontroller_amd import STATELESS, workloads

    stream = torch.cuda.Stream()
    T.first_engine()
    for p in range(args.passes):
        for gen, B, seed in T.WORKLOADS:
            inp = getattr(workloads, gen)(B, seed=seed)
            e = T.engine(inp, None, stream)
            parent = T.engine(inp, args.parent_lib, stream) if args.parent_lib else None
            none, default, seed11 = e.force_bounds(), e.force_task(), FT.table(B, 11, inp["contacts"])

            def form(fn, ft):
                def measure():
                    e.set_force_bounds(fn)
                    e.set_force_task(ft)
                    return T.timed(e, args.steps, args.warmup, stream, STATELESS)
                return measure

            def parent_form(fn):
                def measure():
                    parent.set_force_bounds(fn)
                    return T.timed(parent, args.steps, args.warmup, stream, STATELESS)
                return measure

            forms = [("plain", form(None, None)), ("fn", form(none, None)), ("ft", form(none, default)),
                     ("ft_only", form(None, default)), ("seed11", form(None, seed11))]
            if parent:
                forms += [("parent", parent_form(None)), ("parent_fn", parent_form(none))]
            us = T.rotate(args.rounds, forms)
            e.set_force_bounds(None)
            e.set_force_task(None)
            e.close()
            if parent:
                parent.set_force_bounds(None)
                parent.close()
            T.report({"pass": p, "workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds}, us,
                     lambda m: {"ft_over_fn": T.ratio(m, "ft", "fn"), "ft_only_over_fn": T.ratio(m, "ft_only", "fn"),
                                "seed11_over_ft": T.ratio(m, "seed11", "ft"), "plain_over_parent_plain": T.ratio(m, "plain", "parent"),
                                "fn_over_parent_fn": T.ratio(m, "fn", "parent_fn")}, over_plain=False)


if __name__ == "__main__":
    main()
