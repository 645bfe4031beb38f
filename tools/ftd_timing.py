"""Step time with WBC_DUALS_TASK (the 48 multipliers under a per-robot force task) against the
force-task step without them and against WBC_DUALS_FORCE, on one device in one process: HIP events around
back-to-back launches, as bench.py times a step.

  python tools/ftd_timing.py [--steps 2000] [--warmup 50] [--rounds 5] [--passes 2] [--parent-lib PATH]

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times over:
  ft        (-inf x 4, +inf x 4) and (0 x 12, 1, 0) in every row (wbc_kernel_ft0.hip): the code the new units extend
  fnd       the same force-bound rows, no task, WBC_DUALS_FORCE (wbc_kernel_fnd0.hip)
  ftd       the rows of ft, WBC_DUALS_TASK (wbc_kernel_ftd0.hip)
  ftd_none  no table at all, WBC_DUALS_TASK (ftd0 on the engine's own no-bounds and plain-task tables)
Default rows throughout, so all four solve the same QPs.  With --parent-lib, `parent_ft` and `parent_fnd`: the ft and
fnd steps of another build of the library (the parent commit's) on an engine of its own, in the same rotation, which
gives the noise floor.  The whole run is repeated `passes` times; one JSON line per workload and pass with the median
us per step of each form, ftd over ft (the DU stage's own cost), ftd over fnd (the task's cost under duals), and this
build's ft and fnd steps over the parent's."""
import argparse

import step_timing_common as T


def main():
    ap = argparse.ArgumentParser()
    T.add_timing_arguments(ap, steps=2000, warmup=50, rounds=5)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    import torch

    from quadrupedwholebodycontroller_amd import DUALS_FORCE, DUALS_TASK, STATELESS, workloads

    stream = torch.cuda.Stream()
    T.first_engine()
    for p in range(args.passes):
        for gen, B, seed in T.WORKLOADS:
            inp = getattr(workloads, gen)(B, seed=seed)
            e = T.engine(inp, None, stream)
            parent = T.engine(inp, args.parent_lib, stream) if args.parent_lib else None
            none, default = e.force_bounds(), e.force_task()

            def form(eng, fn, ft, flags):
                def measure():
                    eng.set_force_bounds(fn)
                    eng.set_force_task(ft)
                    return T.timed(eng, args.steps, args.warmup, stream, STATELESS | flags)
                return measure

            forms = [("ft", form(e, none, default, 0)), ("fnd", form(e, none, None, DUALS_FORCE)),
                     ("ftd", form(e, none, default, DUALS_TASK)), ("ftd_none", form(e, None, None, DUALS_TASK))]
            if parent:
                forms += [("parent_ft", form(parent, none, default, 0)), ("parent_fnd", form(parent, none, None, DUALS_FORCE))]
            us = T.rotate(args.rounds, forms)
            for eng in (e, parent):
                if eng:
                    eng.set_force_bounds(None)
                    eng.set_force_task(None)
                    eng.close()
            T.report({"pass": p, "workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds}, us,
                     lambda m: {"ftd_over_ft": T.ratio(m, "ftd", "ft"), "ftd_over_fnd": T.ratio(m, "ftd", "fnd"),
                                "ftd_none_over_ftd": T.ratio(m, "ftd_none", "ftd"), "ft_over_parent_ft": T.ratio(m, "ft", "parent_ft"),
                                "fnd_over_parent_fnd": T.ratio(m, "fnd", "parent_fnd")}, over_plain=False)


if __name__ == "__main__":
    main()
