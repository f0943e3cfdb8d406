#!/usr/bin/env python3
"""Paired timing of the launch orders of the staged float kernel on the bench workload: one process, one plan, both batches placed
by the library as bench.py takes them, the tuning build switching the order between launches (FIMEX_AMD_STAGE2_ORDER 1 / 2).

  paired_orders.py [--method bilinear] [--nz 200] [--launches 30] [--cohort 8x4] [--out FILE]

The plan is tuned first (fimex_amd_regrid_plan_tune_device: shape, then order, by its 1 % rule; what it chose is reported), then
the two orders alternate, `launches` timed launches each after two untimed ones.  Reported: median and min per order, and of the
paired differences (tile-major minus chunk-per-XCD, launch k against launch k) the median and the median absolute deviation.  The
outputs of the two orders are compared byte for byte.  Prints one JSON line, appends it to --out."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--method", default="bilinear", choices=["bilinear", "nearest", "bicubic"])
    ap.add_argument("--nz", type=int, default=200)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--cohort", default="8x4", help="bands x tiles of a cohort (read when the plan is built)")
    ap.add_argument("--workload", default="default", choices=["default", "one_percent"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from fimex_amd import capi as fa
    import bench
    import workloads
    by, bx = a.cohort.split("x")
    os.environ["FIMEX_AMD_STAGE2_COHORT_BANDS"], os.environ["FIMEX_AMD_STAGE2_COHORT_TILES"] = by, bx
    fa.use_tuning_build(True)
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    wl = workloads.BilinearRotatedPole(variant=a.workload)
    method = {"bilinear": fa.BILINEAR, "nearest": fa.NEAREST_NEIGHBOR, "bicubic": fa.BICUBIC}[a.method]
    plan = bench.build_plan(fa, torch, wl, method, st, bicubic=fa.BICUBIC_FAST if a.method == "bicubic" else None)[0]
    src = plan.alloc_source_batch(a.nz, candidates=6, stream=st)
    d_in = bench.make_slices(torch, wl.base_field(), a.nz, 0, into=src.as_tensor())
    torch.cuda.synchronize()
    batch = plan.alloc_batch(d_in.data_ptr(), a.nz, positions=8, stream=st)
    d_out = batch.as_tensor()
    shape = plan.tune_device(d_in.data_ptr(), a.nz, d_out.data_ptr(), st)
    tuned = {"shape": shape, "launchOrder": plan.info()["launchOrder"], "tile": [plan.info()["tileW"], plan.info()["tileH"]]}

    def launch(order):
        os.environ["FIMEX_AMD_STAGE2_ORDER"] = str(order)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.apply_device(d_in.data_ptr(), a.nz, d_out.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    taken = {}
    for order in (1, 2):
        os.environ["FIMEX_AMD_STAGE2_ORDER"] = str(order)
        taken[order] = plan.launch_order(a.nz)
    sha = {}
    for order in (1, 2):
        d_out.fill_(7.0)
        launch(order)
        sha[order] = hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()
    ms = {1: [], 2: []}
    for k in range(a.launches + 2):
        for order in ((1, 2) if k % 2 == 0 else (2, 1)):  # who goes first alternates too
            t = launch(order)
            if k >= 2:
                ms[order].append(t)
    t1, t2 = np.array(ms[1]), np.array(ms[2])
    d = t1 - t2
    res = {"method": a.method, "nz": a.nz, "workload": a.workload, "cohort": a.cohort, "launches_each": a.launches, "device": torch.cuda.get_device_name(0),
           "tune_device_chose": tuned, "order_taken": {"STAGE2_ORDER=1": taken[1], "STAGE2_ORDER=2": taken[2]},
           "same_bytes": sha[1] == sha[2],
           "tile_major_ms": {"median": float(np.median(t1)), "min": float(t1.min())},
           "chunk_per_xcd_ms": {"median": float(np.median(t2)), "min": float(t2.min())},
           "paired_difference_ms": {"median": float(np.median(d)), "mad": float(np.median(np.abs(d - np.median(d)))), "min": float(d.min()),
                                    "max": float(d.max())},
           "gain_percent_of_tile_major_median": float(100 * (np.median(t1) - np.median(t2)) / np.median(t1))}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    del d_out
    batch.close()
    src.close()


if __name__ == "__main__":
    main()
