#!/usr/bin/env python3
"""Times the staged regrid launches of two builds of the library against each other on the benchmark geometry.

  compare_staged2_builds.py --parent DIR [--rounds 5] [--out profiles/staged2_split_parent_vs_new.json]

DIR holds libfimex_amd.so built from the commit to compare with; the other side is the library of this tree.  The two sides
alternate, one fresh process per side and round, each process runs every case: bilinear (the bench.py headline), nearest and
bicubic in float arithmetic on 200 float slices, bilinear on int16 and nearest on uint8 on 200 slices, bilinear on 25 slices, bicubic
in the reference's arithmetic on 200 slices (the first staged form's production launch), and the creation of the bilinear plan from
positions on the device (wall time, its host round trips included).  One untimed case hashes what info() says of every plan the
script builds (planBytes, stagedCells, tileW, tileH, undefined and border cells): equal planBytes means equal tile count, chunk
total and table length.
Per case and round the minimum of three timed launches counts, then the median over the rounds.  Margin: new median - parent
median <= the parent's own (max - min) over its rounds.  A sha256 of the output bytes per case must be the same on both sides in
every round.  The driver (compare_builds.py) stops at the first process that does not end normally.
"""
import argparse, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compare_builds  # beside this script

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
compare_builds.add_arguments(ap, os.path.join(ROOT, "profiles", "staged2_split_parent_vs_new.json"))
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

    infos = {}

    def built(name, plan):
        i = plan.info()
        infos[name] = {k: i[k] for k in ("planBytes", "stagedCells", "tileW", "tileH", "undefinedCells", "borderCells")}
        return plan

    bilinear, px, py = bench.build_plan(fa, torch, wl, fa.BILINEAR, st)
    built("bilinear", bilinear)
    floats("bilinear_nz200", bilinear, 200)
    floats("bilinear_nz25", bilinear, 25)
    stored("bilinear_int16_nz200", bilinear, d_i16, fa.CDM_SHORT, -32767.0)
    nearest = built("nearest", bench.build_plan(fa, torch, wl, fa.NEAREST_NEIGHBOR, st)[0])
    floats("nearest_nz200", nearest, 200)
    stored("nearest_uint8_nz200", nearest, d_u8, fa.CDM_UCHAR, 255.0)
    cubic = built("bicubic_float", bench.build_plan(fa, torch, wl, fa.BICUBIC, st, bicubic=fa.BICUBIC_FAST)[0])
    floats("bicubic_float_nz200", cubic, 200)
    del cubic
    cubic = built("bicubic_reference", bench.build_plan(fa, torch, wl, fa.BICUBIC, st, bicubic=fa.BICUBIC_REFERENCE)[0])
    floats("bicubic_reference_nz200", cubic, 200)
    del cubic

    # plan creation from positions that are on the device already
    d_px, d_py = torch.from_numpy(px).cuda(), torch.from_numpy(py).cuda()
    ts = []
    for k in range(5):  # two untimed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = fa.RegridPlan.from_device(fa.BILINEAR, d_px.data_ptr(), d_py.data_ptr(), d_px.numel(), wl.inX, wl.inY, wl.outX, wl.outY, st)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        built("bilinear_again_%d" % k, plan)
        del plan
    print(json.dumps({"case": "bilinear_plan_create", "seconds": ts[2:],
                      "sha256": hashlib.sha256(json.dumps(infos["bilinear_again_4"], sort_keys=True).encode()).hexdigest()}), flush=True)
    print(json.dumps({"case": "plan_info", "sha256": hashlib.sha256(json.dumps(infos, sort_keys=True).encode()).hexdigest(), "info": infos}), flush=True)


WHAT = "Staged regrid launches on the benchmark geometry."


worker() if args.worker else compare_builds.drive(__file__, args, WHAT)
