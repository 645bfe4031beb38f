"""Step time with WBC_DUALS_FORCE (the 48 multipliers under per-foot force bounds) against the
force-bound step and the limits duals step it stands beside, on one device in one process: HIP events around
back-to-back launches, as bench.py times a step.

  python tools/force_duals_timing.py [--steps 2000] [--warmup 50] [--rounds 5] [--passes 2] [--parent-lib PATH]

Per workload (stance_cold B = 4096, rl_random B = 8192) one engine runs, in turn and `rounds` times over, under
uniform limits rows (-max_torque x 12, +max_torque x 12, friction x 4):
  plain     no table at all (wbc_kernel_stance.hip / wbc_kernel_step0.hip)
  lmd       the limits rows, WBC_DUALS (wbc_kernel_lmd0.hip)
  fn        the limits rows and (-inf x 4, +inf x 4) in every row (wbc_kernel_fn0.hip)
  fnd       the same tables, WBC_DUALS_FORCE (wbc_kernel_fnd0.hip): the same QPs as fn and lmd
  fnd_none  the limits rows, no force-bound table, WBC_DUALS_FORCE (fnd0 on the engine's own no-bounds table)
  fnd_seed7 the limits rows and tests/force_bounds_oracle.py table(B, 7), WBC_DUALS_FORCE: other QPs
and, with --parent-lib, `parent`, `parent_fn` and `parent_lmd`: the plain, the force-bound and the limits duals
step of another build of the library (the parent commit's) on an engine of its own, in the same rotation.  The whole
run is repeated `passes` times; one JSON line per workload and pass with the median us per step of each form, fnd
over fn and over lmd (the new stage's own cost), and this build's plain, fn and lmd steps over the parent's (the
parent's spread in the same session)."""
import argparse

import step_timing_common as T


def main():
    ap = argparse.ArgumentParser()
    T.add_timing_arguments(ap, steps=2000, warmup=50, rounds=5)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    import torch

    import force_bounds_oracle as FO
    from quadrupedwholebodycontroller_amd import DUALS, DUALS_FORCE, STATELESS, workloads

    stream = torch.cuda.Stream()
    T.first_engine()
    for p in range(args.passes):
        for gen, B, seed in T.WORKLOADS:
            inp = getattr(workloads, gen)(B, seed=seed)
            e = T.engine(inp, None, stream)
            parent = T.engine(inp, args.parent_lib, stream) if args.parent_lib else None
            uniform, none, seed7 = e.limits(), e.force_bounds(), FO.table(B)

            def form(eng, lm, fn, flags):
                def measure():
                    eng.set_limits(lm)
                    eng.set_force_bounds(fn)
                    return T.timed(eng, args.steps, args.warmup, stream, STATELESS | flags)
                return measure

            forms = [("plain", form(e, None, None, 0)), ("lmd", form(e, uniform, None, DUALS)), ("fn", form(e, uniform, none, 0)),
                     ("fnd", form(e, uniform, none, DUALS_FORCE)), ("fnd_none", form(e, uniform, None, DUALS_FORCE)),
                     ("fnd_seed7", form(e, uniform, seed7, DUALS_FORCE))]
            if parent:
                forms += [("parent", form(parent, None, None, 0)), ("parent_fn", form(parent, uniform, none, 0)),
                          ("parent_lmd", form(parent, uniform, None, DUALS))]
            us = T.rotate(args.rounds, forms)
            for eng in (e, parent):
                if eng:
                    eng.set_limits(None)
                    eng.set_force_bounds(None)
                    eng.close()
            T.report({"pass": p, "workload": gen, "batch": B, "steps": args.steps, "rounds": args.rounds}, us,
                     lambda m: {"fnd_over_fn": T.ratio(m, "fnd", "fn"), "fnd_over_lmd": T.ratio(m, "fnd", "lmd"),
                                "fnd_none_over_fnd": T.ratio(m, "fnd_none", "fnd"), "fnd_seed7_over_fnd": T.ratio(m, "fnd_seed7", "fnd"),
                                "plain_over_parent_plain": T.ratio(m, "plain", "parent"), "fn_over_parent_fn": T.ratio(m, "fn", "parent_fn"),
                                "lmd_over_parent_lmd": T.ratio(m, "lmd", "parent_lmd")}, over_plain=False)


if __name__ == "__main__":
    main()
