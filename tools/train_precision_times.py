#!/usr/bin/env python
"""What does a training step cost under each operand precision of the training convs?  For one configuration of
tools/train_determinism.py, ONE model takes steps (p_losses + backward, dropout on, both loss terms, default mode) under
train precision 32, 16 ("bf16-mixed") and 48 ("bf16x3"), the three alternating in one process; prints ONE JSON line with the median
and the range of `--reps` steps each, and the ratios to the fp32 step.

    python tools/train_precision_times.py --config ns    [--rows 32]   # NS shapes: unet_simple dim 64 @ 256^2
    python tools/train_precision_times.py --config oisst [--rows 64]   # OISST shapes: unet.Unet dim 64, mults (1, 2, 4)

Needs an MI355X.  Imports neither the oracle nor the reference.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.train_determinism import make, step  # noqa: E402

PRECISIONS = (32, 16, 48)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", choices=["ns", "oisst"], default="ns")
    ap.add_argument("--rows", type=int, default=None, help="batch rows of the step (ns 32, oisst 64)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="timed steps per precision")
    a = ap.parse_args()
    rows = a.rows or {"ns": 32, "oisst": 64}[a.config]
    m, batch = make(a.config, rows, 32)
    step(m, batch, False, a.seed)  # builds the engine
    eng = m._engine
    times, loss = {p: [] for p in PRECISIONS}, {}
    for p in PRECISIONS:  # warm every precision: first-use allocations, the raised LDS limits
        eng.train_set_precision(p)
        step(m, batch, False, a.seed)
    for _ in range(a.reps):
        for p in PRECISIONS:
            eng.train_set_precision(p)
            dt, loss[p], _ = step(m, batch, False, a.seed)
            times[p].append(1e3 * dt)
    res = dict(config=a.config, rows=rows, seed=a.seed, reps=a.reps)
    for p in PRECISIONS:
        res[f"ms_per_step_{p}"] = round(statistics.median(times[p]), 2)
        res[f"ms_range_{p}"] = [round(min(times[p]), 2), round(max(times[p]), 2)]
        res[f"loss_{p}"] = loss[p]
    for p in (16, 48):
        res[f"time_{p}_over_32"] = round(res[f"ms_per_step_{p}"] / res["ms_per_step_32"], 4)
    m.eval()
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
