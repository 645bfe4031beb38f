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

import step_timing_common as T


def main():
    ap = argparse.ArgumentParser()
    T.add_timing_arguments(ap, steps=200, warmup=20, rounds=7)
    ap.add_argument("--states", type=int, default=1024)
    args = ap.parse_args()
    import torch

    from quadrupedwholebodycontroller_amd import BEST, NO_X, OBJECTIVE, STATELESS, workloads

    stream = torch.cuda.Stream()
    inp, modes = workloads.mode_states(args.states, 4)
    T.first_engine()
    e = T.engine(inp, None, stream, modes)
    parent = T.engine(inp, args.parent_lib, stream, modes) if args.parent_lib else None

    def form(eng, flags):
        return lambda: T.timed(eng, args.steps, args.warmup, stream, flags, eng.step_modes)

    base = STATELESS | NO_X
    forms = [("plain", form(e, base)), ("objective", form(e, base | OBJECTIVE)), ("best", form(e, base | BEST)),
             ("plain_x", form(e, STATELESS)), ("objective_x", form(e, STATELESS | OBJECTIVE))]
    if parent:
        forms.append(("parent", form(parent, base)))
    us = T.rotate(args.rounds, forms, (["parent"] if parent else []) + [name for name, _ in forms[:5]])  # the parent first
    m = e.modes_per_wave()
    e.close()
    if parent:
        parent.close()
    T.report({"workload": "mode_states", "states": args.states, "modes": len(modes), "batch": args.states * len(modes),
              "modes_per_wave": m, "steps": args.steps, "rounds": args.rounds}, us,
             lambda med: {"best_minus_objective_us": round(med["best"] - med["objective"], 3),
                          "objective_over_plain_x": T.ratio(med, "objective", "plain_x"),
                          "objective_x_over_plain_x": T.ratio(med, "objective_x", "plain_x")})


if __name__ == "__main__":
    main()
