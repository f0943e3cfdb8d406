#!/usr/bin/env python3
"""Times the staged regrid launches of two builds of the library against each other on the benchmark geometry.

  compare_staged2_builds.py --parent DIR [--rounds 5] [--out profiles/staged2_split_parent_vs_new.json]

DIR holds libfimex_amd.so built from the commit to compare with; the other side is the library of this tree.  The two sides
alternate, one fresh process per side and round, each process runs every case: bilinear (the bench.py headline), nearest and
bicubic in float arithmetic on 200 float slices, bilinear on int16 and nearest on uint8 on 200 slices, bilinear on 25 slices.
Per case and round the minimum of three timed launches counts, then the median over the rounds.  Margin: new median - parent
median <= the parent's own (max - min) over its rounds.  A sha256 of the output bytes per case must be the same on both sides in
every round.  The driver stops at the first process that does not end normally.
"""
import argparse, hashlib, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--parent", help="directory with the other build's libfimex_amd.so")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staged2_split_parent_vs_new.json"))
ap.add_argument("--parent-commit", default="parent")
ap.add_argument("--worker", action="store_true", help="one side, one round: prints a JSON line per case")
ap.add_argument("--lib", default=None, help="worker: directory of the library to load instead of this tree's")
args = ap.parse_args()


def worker():
    import numpy as np
    import torch
    from fimex_amd import capi as fa
    import workloads, bench
    if args.lib:
        fa.LIB_PATH = os.path.join(args.lib, "libfimex_amd.so")
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    wl = workloads.BilinearRotatedPole()
    d_f = bench.make_slices(torch, wl.base_field(), 200)
    d_i16 = (torch.nan_to_num(d_f, nan=-327.67) * 100).to(torch.int16)
    d_u8 = (torch.nan_to_num(d_f, nan=255.0).abs() % 255).to(torch.uint8)

    def timed(name, launch, d_out):
        for _ in range(2): launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); launch(); b.record()
            torch.cuda.synchronize(); ts.append(a.elapsed_time(b) / 1e3)
        print(json.dumps({"case": name, "seconds": ts, "sha256": hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()}), flush=True)

    def floats(name, plan, nz):
        d_out = torch.empty((nz, wl.outY, wl.outX), dtype=torch.float32, device="cuda")
        timed(name, lambda: plan.apply_device(d_f.data_ptr(), nz, d_out.data_ptr(), st), d_out)

    def stored(name, plan, d_in, code, bad):
        d_out = torch.empty((200, wl.outY, wl.outX), dtype=d_in.dtype, device="cuda")
        timed(name, lambda: fa.regrid_apply_typed_device(plan, d_in.data_ptr(), code, 200, bad, d_out.data_ptr(), st), d_out)

    bilinear, _, _ = bench.build_plan(fa, torch, wl, fa.BILINEAR, st)
    floats("bilinear_nz200", bilinear, 200)
    floats("bilinear_nz25", bilinear, 25)
    stored("bilinear_int16_nz200", bilinear, d_i16, fa.CDM_SHORT, -32767.0)
    nearest, _, _ = bench.build_plan(fa, torch, wl, fa.NEAREST_NEIGHBOR, st)
    floats("nearest_nz200", nearest, 200)
    stored("nearest_uint8_nz200", nearest, d_u8, fa.CDM_UCHAR, 255.0)
    cubic, _, _ = bench.build_plan(fa, torch, wl, fa.BICUBIC, st, bicubic=fa.BICUBIC_FAST)
    floats("bicubic_float_nz200", cubic, 200)


def driver():
    sides = {"parent": ["--lib", os.path.abspath(args.parent)], "new": []}
    runs = {s: {} for s in sides}  # side -> case -> list of rounds
    for rnd in range(args.rounds):
        for side, extra in sides.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + extra, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("round %d, %s: exit %d\n%s" % (rnd, side, r.returncode, r.stderr[-2000:]))
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    c = json.loads(line)
                    runs[side].setdefault(c["case"], []).append(c)
            print("round", rnd, side, "done", flush=True)
    cases, ok = {}, True
    for case in runs["new"]:
        e = {}
        for side in sides:
            mins = [min(c["seconds"]) for c in runs[side][case]]
            e[side] = {"rounds_seconds_min": mins, "rounds_seconds_all": [c["seconds"] for c in runs[side][case]], "median": statistics.median(mins),
                       "spread": max(mins) - min(mins), "sha256": sorted({c["sha256"] for c in runs[side][case]})}
        e["new_minus_parent"] = e["new"]["median"] - e["parent"]["median"]
        e["within_margin"] = e["new_minus_parent"] <= e["parent"]["spread"]
        e["same_bits"] = len(e["parent"]["sha256"]) == 1 and e["parent"]["sha256"] == e["new"]["sha256"]
        ok = ok and e["within_margin"] and e["same_bits"]
        cases[case] = e
        print(case, "parent %.4f ms  new %.4f ms  margin %.4f ms  same bits %s" % (e["parent"]["median"] * 1e3, e["new"]["median"] * 1e3,
                                                                                  e["parent"]["spread"] * 1e3, e["same_bits"]), flush=True)
    what = ("staged regrid launches on the benchmark geometry, commit %s against this tree, alternating in one GPU call: one fresh process per "
            "side and round runs every case; per case and round the minimum of three launches, then the median over rounds.  Margin: new median - "
            "parent median <= parent's (max - min) over its rounds.  sha256: of the output batch's bytes after the last launch; one value on both "
            "sides means the same bits in every round." % args.parent_commit)
    with open(args.out, "w") as f:
        json.dump({"what": what, "device": "MI355X", "rounds": args.rounds, "all_within_margin_and_same_bits": ok, "cases": cases}, f, indent=1)
        f.write("\n")
    print("all within margin and same bits:", ok, flush=True)


worker() if args.worker else driver()
