#!/usr/bin/env python3
"""The entries of SURVEY 8f n11, device-resident and HIP-event timed, in one call.
  extraction    65 levels of a 4000 x 3000 source:
                  crop          x 1001..3000 (an odd offset), y 500..2499, as float and as packed short
                  levels        10 of the 65 levels over whole planes, float
                  every second  every second x and every second y, float
                  date line     the two x runs 0..499 and 3500..3999 of a box across 180 degrees, y 500..2499, float
                each next to a device copy of the output's bytes (which moves the touched bytes, 2 x output bytes) and next to what
                a user of torch does today: .contiguous() of the sliced view for the crop, torch.index_select (one call per picked
                dimension) for the others.  The results are compared bit for bit once.
  bounding box  fimex_amd_extract_bounding_box_host on a 2000 x 2000 mesh, rotated pole and lcc: wall time of the call, which ends
                with the positions on the host, next to fimex_amd_project_axes_device for the same mesh, which leaves the two
                projected [iy][ix] fields on the device (wall time up to the end of the stream).
Within a case the candidates alternate, call by call, so that a drift of the machine hits all of them alike; the figures are medians
over --launches rounds after 3 warm-up rounds, and the spread is (max - min) / median of those rounds.  Writes profiles/extract.json
(or --out) and prints one JSON line per case.

usage: python scripts/bench_extract.py [--launches 20] [--out FILE]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX, NY, NZ = 4000, 3000, 65
LONLAT = "+proj=latlong +R=6.371e+06"
ROT = "+proj=ob_tran +o_proj=longlat +lon_0=-40 +o_lat_p=22 +R=6.371e+06 +no_defs"
LCC = "+proj=lcc +lat_0=63 +lon_0=15 +lat_1=63 +lat_2=63 +no_defs +R=6.371e+06"


def alternating(torch, fns, reps, warm=3):
    """{name: (median ms, min ms, max ms)} of the callables, one call of each per round."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def wall(torch, fns, reps, warm=3):
    """The same with the host's clock around call and synchronisation."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def stats(t, k):
    return {k + "_ms_median": t[k][0], k + "_ms_min": t[k][1], k + "_ms_max": t[k][2], k + "_spread": (t[k][2] - t[k][1]) / t[k][0]}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract.json"))
    args = ap_.parse_args()
    import torch
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    device = torch.cuda.get_device_name(0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    results = []

    src_f = torch.randn((NZ, NY, NX), device="cuda", generator=gen)
    src_s = torch.randint(-20000, 20000, (NZ, NY, NX), dtype=torch.int16, device="cuda", generator=gen)
    levels = np.array([0, 3, 4, 10, 20, 21, 22, 40, 50, 64])
    xs2, ys2 = np.arange(0, NX, 2), np.arange(0, NY, 2)
    xruns = np.concatenate([np.arange(0, 500), np.arange(3500, 4000)])

    def dev(a):
        return torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()

    d_levels, d_xs2, d_ys2, d_xruns = dev(levels), dev(xs2), dev(ys2), dev(xruns)
    cases = [
        ("crop, float", src_f, fa.CDM_FLOAT, [(NX, None, 1001, 2000), (NY, None, 500, 2000), (NZ, None)],
         lambda s: s[:, 500:2500, 1001:3001].contiguous(), ".contiguous() of the sliced view"),
        ("crop, packed short", src_s, fa.CDM_SHORT, [(NX, None, 1001, 2000), (NY, None, 500, 2000), (NZ, None)],
         lambda s: s[:, 500:2500, 1001:3001].contiguous(), ".contiguous() of the sliced view"),
        ("10 of 65 levels, float", src_f, fa.CDM_FLOAT, [(NX, None), (NY, None), (NZ, levels)],
         lambda s: s.index_select(0, d_levels), "index_select(0)"),
        ("every second x and y, float", src_f, fa.CDM_FLOAT, [(NX, xs2), (NY, ys2), (NZ, None)],
         lambda s: s.index_select(1, d_ys2).index_select(2, d_xs2), "index_select(1) then index_select(2)"),
        ("two x runs across the date line, float", src_f, fa.CDM_FLOAT, [(NX, xruns), (NY, None, 500, 2000), (NZ, None)],
         lambda s: s[:, 500:2500].index_select(2, d_xruns), "index_select(2) of the y slice"),
    ]
    for label, src, code, dims, torch_fn, torch_what in cases:
        plan = fa.ExtractPlan(dims)
        n, elem = plan.info.outElements, src.element_size()
        out = torch.empty(plan.shape, dtype=src.dtype, device="cuda")
        c_src = torch.zeros(n * elem, dtype=torch.uint8, device="cuda"); c_dst = torch.empty_like(c_src)
        keep = {}
        fns = {"extract": lambda: plan.apply_device(src.data_ptr(), code, out.data_ptr(), stream=st),
               "copy": lambda: c_dst.copy_(c_src),
               "torch": lambda: keep.__setitem__("t", torch_fn(src))}
        t = alternating(torch, fns, args.launches)
        fns["extract"](); fns["torch"](); torch.cuda.synchronize()
        identical = bool(torch.equal(out.view(torch.uint8), keep["t"].contiguous().view(torch.uint8)))
        touched = 2 * n * elem
        r = {"case": label, "source": [NZ, NY, NX], "output": list(plan.shape), "element_bytes": elem, "launches": args.launches,
             "kernelDims": plan.info.kernelDims, "fastestRuns": plan.info.fastestRuns, "touched_bytes": touched,
             "touched_bytes_formula": "2 * output bytes", "extract_TBps_of_touched": touched / t["extract"][0] / 1e9,
             "copy_TBps": touched / t["copy"][0] / 1e9, "extract_over_copy": t["extract"][0] / t["copy"][0], "torch_does": torch_what,
             "extract_over_torch": t["extract"][0] / t["torch"][0], "extract_equals_torch_bit_for_bit": identical, "device": device}
        for k in fns:
            r.update(stats(t, k))
        print(json.dumps(r), flush=True)
        results.append(r)
        del plan, out, c_src, c_dst, keep
    del src_f, src_s

    # ---- bounding box
    m = 2000
    out_x = torch.empty((m, m), dtype=torch.float64, device="cuda"); out_y = torch.empty_like(out_x)
    for label, proj, xa, ya, degree, box in (
            ("rotated pole", ROT, np.linspace(-20.0, 20.0, m), np.linspace(-15.0, 15.0, m), True, (55.0, 65.0, 0.0, 20.0)),
            ("lcc", LCC, (np.arange(m) - m / 2) * 2500.0, (np.arange(m) - m / 2) * 2500.0, False, (58.0, 66.0, 5.0, 25.0))):
        ax, ay = (np.radians(xa), np.radians(ya)) if degree else (xa, ya)
        got = {}
        fns = {"bounding_box": lambda: got.__setitem__("p", fa.extract_bounding_box_host(proj, LONLAT, xa, ya, *box, axesInDegree=degree)),
               "project_axes": lambda: fa.project_axes_device(proj, LONLAT, ax, ay, out_x.data_ptr(), out_y.data_ptr(), stream=st)}
        t = wall(torch, fns, args.launches)
        lon, lat = np.degrees(out_x.cpu().numpy()), np.degrees(out_y.cpu().numpy())
        inside = (lat >= box[0]) & (lat <= box[1]) & (lon >= box[2]) & (lon <= box[3])
        agree = bool(np.array_equal(got["p"][0], np.flatnonzero(inside.any(axis=0))) and np.array_equal(got["p"][1], np.flatnonzero(inside.any(axis=1))))
        r = {"case": "bounding box, " + label, "mesh": [m, m], "box_south_north_west_east": list(box), "launches": args.launches,
             "x_kept": int(got["p"][0].size), "y_kept": int(got["p"][1].size), "positions_agree_with_the_projected_fields": agree,
             "timing": "host clock around the call and the synchronisation", "bounding_box_returns": "the positions on the host",
             "project_axes_returns": "two [iy][ix] double fields on the device (%d bytes)" % (2 * 8 * m * m),
             "bounding_box_over_project_axes": t["bounding_box"][0] / t["project_axes"][0], "device": device}
        for k in fns:
            r.update(stats(t, k))
        print(json.dumps(r), flush=True)
        results.append(r)

    doc = {"script": "scripts/bench_extract.py",
           "timing": "extraction: HIP events around one call; bounding box: the host's clock around call and synchronisation; the candidates "
                     "of a case alternate call by call; median of the rounds after 3 warm-up rounds; spread = (max - min) / median of the rounds",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
