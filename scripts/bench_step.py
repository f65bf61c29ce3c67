#!/usr/bin/env python
"""Fused post-backward step figures, one JSON line per row count, in the train_single.py
configuration: statistics from raw radii, head lock of all six tensors, select="opacity_grad", the size clamp.

  fused_ms   hgs.step.post_backward_tensors: one select and one apply launch, nothing comes back to the host
  spec_ms    tests/step_spec.py in float32 with hgs.optim.Adam.step(relevant): the reference's call shape (indexed
             statistics, six slice assignments, nonzero(), the optimizer step, boolean-mask clamp) on code that exists
             without hgs.step.  It is NOT the reference's own loop, which cannot be run here.
  The statement's cost is largely host waits, so the figure is the HOST clock around call + stream synchronise; warm-up
  first, the two alternated over --reps repetitions: minimum, median, maximum.  Gradients are re-attached outside the
  clock (both sides set them to None).
  bytes      the traffic floor of the fused call: apply 28 B per updated element + the class byte of every row once per
             tensor (6 B per row) + 12 B per scaling row that is not updated (the clamp reads every row); select 4 B
             opacity gradient + 1 B class per row, 4 B radius per rendered row, 8 B of means2D gradient and 3 x 8 B of
             read-modify-write per visible row
  bound_us   bytes over the measured HBM rate (6.29 TB/s, float4 copy)

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--only fused --reps 2).

    python scripts/bench_step.py [--rows 375000 1000000 8000000] [--K 15] [--visible 0.3] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hierarchical-3d-gaussians_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hgs import step                                 # noqa: E402
import step_cases as sc                              # noqa: E402
from step_spec import NAMES, post_backward_spec      # noqa: E402

HBM_BYTES_PER_S = 6.29e12
SKYBOX = 10_000


def stats(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", type=int, default=[375_000, 1_000_000, 8_000_000])
    ap.add_argument("--K", type=int, default=15)
    ap.add_argument("--visible", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["fused", "spec"], default=None, help="time one side only (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f10_step_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_step.py needs a GPU")
    dev = torch.device("cuda:0")
    lines = []
    for P in args.rows:
        model = sc.make_model(P, args.K, 0, dev, visible_fraction=args.visible)
        # 2 % of the rows violate the size limit (the clamp is a correction, not the common case)
        thr = float(torch.exp(model["params"]["scaling"]).max(dim=1).values.quantile(0.98))
        sc.clear_band(model["params"]["scaling"], thr)
        sides = {}
        for k in ("fused", "spec"):
            if args.only in (None, k):
                params, opt = sc.build(model, 1)
                grads = {n: params[n].grad for n in NAMES}
                st = {s: model[s].clone() for s in ("max_radii2D", "accum", "denom")}
                sides[k] = (params, opt, grads, st)
        del model["params"]

        def attach(k):
            params, _, grads, _ = sides[k]
            for n in NAMES:
                params[n].grad = grads[n]

        def call(k):
            params, opt, grads, st = sides[k]
            if k == "fused":
                step.post_backward_tensors(params, opt, radii=model["radii"], means2D_grad=model["means2D_grad"],
                                           lock_head=SKYBOX, clamp=(thr, 0), **st)
            else:
                post_backward_spec({n: p.data for n, p in params.items()}, grads, optimizer=opt, radii=model["radii"],
                                   means2D_grad=model["means2D_grad"], lock_head=SKYBOX, clamp_args=(thr, 0), **st)

        def timed(k):
            attach(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(k)
            torch.cuda.current_stream().synchronize()
            return (time.perf_counter() - t0) * 1e3
        for _ in range(args.warmup):
            for k in sides:
                timed(k)
        host = {k: [] for k in sides}
        for _ in range(args.reps):
            for k in sides:
                host[k].append(timed(k))
        n_vis = int(model["visible"].numel())
        n_sel = int((sides[next(iter(sides))][2]["opacity"].flatten()[SKYBOX:] != 0).sum())
        row_floats = 14 + 3 * args.K
        apply_bytes = n_sel * row_floats * 28 + (P - n_sel) * 12 + P * 6
        select_bytes = P * (4 + 1) + P * 4 + n_vis * (8 + 3 * 8)
        nbytes = apply_bytes + select_bytes
        row = {"rows": P, "K": args.K, "visible_rows": n_vis, "selected_rows": n_sel, "reps": args.reps,
               "clamp_threshold": thr, "bytes": nbytes, "apply_bytes": apply_bytes, "select_bytes": select_bytes,
               "bound_us": nbytes / HBM_BYTES_PER_S * 1e6}
        for k in sides:
            row[f"{k}_ms"] = stats(host[k])
        if len(sides) == 2:
            row["speedup_median"] = row["spec_ms"]["median"] / row["fused_ms"]["median"]
            row["speedup_worst"] = row["spec_ms"]["min"] / row["fused_ms"]["max"]
            row["ranges_overlap"] = row["fused_ms"]["max"] >= row["spec_ms"]["min"]
        if "fused" in sides:
            row["byte_bound_share"] = row["bound_us"] / (row["fused_ms"]["median"] * 1e3)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
        del sides, model
        torch.cuda.empty_cache()
    if args.out and not args.only:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
