"""What the step-timing tools share (cn_timing.py, bb_timing.py, duals_timing.py, lm_timing.py, fn_timing.py,
ft_timing.py, ftd_timing.py, modes_obj_timing.py): an engine on a stream, of this build or of another build's library; HIP events around
back-to-back steps, as bench.py times a step; the rotation of the forms over the rounds; the JSON line; and the
numpy oracles' active-set passes.  Each tool keeps its forms, its ratios and its command line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WORKLOADS = (("stance_cold", 4096, 1), ("rl_random", 8192, 3))


def add_timing_arguments(ap, steps, warmup, rounds):
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--parent-lib", default=None)


def engine(inp, lib_path, stream, modes=None):
    """An engine on `stream` loaded with `inp` (under a mode list, one hypothesis per state and mode); with
    `lib_path`, an engine of another build: its own library handle, this build's Python wrapper."""
    from quadrupedwholebodycontroller_amd import Engine, _capi

    B = len(inp["contacts"]) * (len(modes) if modes is not None else 1)
    if lib_path:
        own, _capi._lib = _capi._lib, None
        try:
            _capi.load_library(os.path.abspath(lib_path))
            e = Engine(B)
        finally:
            _capi._lib = own
    else:
        e = Engine(B)
    e.set_stream(stream)
    if modes is not None:
        e.set_modes(modes)
    e.set_state(inp["base_pose"], inp["nu"], inp["qj"])
    e.set_reference(inp["ref"], inp["contacts"], inp["switching"])
    return e


def first_engine():
    """This build's library becomes the process's default before another one is loaded."""
    from quadrupedwholebodycontroller_amd import Engine

    Engine(4).close()


def timed(e, steps, warmup, stream, flags, step=None):
    """us per step of `steps` back-to-back e.step(flags) (or step(flags)) after `warmup` of them."""
    import torch

    step = step or e.step
    for _ in range(warmup):
        step(flags)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for _ in range(steps):
        step(flags)
    ev1.record(stream)
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps * 1e3


def rotate(rounds, forms, order=None):
    """forms: [(name, measure)], measure() setting its form up and returning one timing.  Every form in turn (in
    `order`, a list of names, else as listed), `rounds` times over: {name: [timings]} in the forms' order."""
    us = {name: [] for name, _ in forms}
    measure = dict(forms)
    for _ in range(rounds):
        for name in order or us:
            us[name].append(measure[name]())
    return us


def ratio(med, a, b):
    """med[a] / med[b], or None where one of them was not measured (no --parent-lib)."""
    return round(med[a] / med[b], 4) if a in med and b in med else None


def report(head, us, ratios, over_plain=True):
    """One JSON line: `head`, the medians and the min / max over the rounds, each median over the plain step's,
    and the tool's own figures ratios(med)."""
    med = {k: float(np.median(v)) for k, v in us.items()}
    line = {**head,
            "us_per_step": {k: round(v, 3) for k, v in med.items()},
            "us_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in us.items()}}
    if over_plain:
        line["over_plain"] = {k: round(v / med["plain"], 4) for k, v in med.items()}
    print(json.dumps({**line, **ratios(med)}), flush=True)


def oracle_passes(n, tables, run_batch, tight):
    """No GPU: per workload, the numpy oracle's active-set passes on n robots under each (name, table) of
    tables(n); tight(result, table, inputs): the robots on which a bound of the table is tight."""
    from quadrupedwholebodycontroller_amd import workloads

    for gen, _, seed in WORKLOADS:
        inp = getattr(workloads, gen)(n, seed=seed)
        res = {}
        for name, t in tables(n):
            r = run_batch(inp, t)
            res[name] = dict(ok=int((r["status"] == 0).sum()), mean_passes=round(float(r["iters"].mean()), 3),
                             max_passes=int(r["iters"].max()), tight=tight(r, t, inp))
        print(json.dumps({"workload": gen, "robots": n, **res}), flush=True)
