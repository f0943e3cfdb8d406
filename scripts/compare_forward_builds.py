#!/usr/bin/env python3
"""Compares the forward regrid of two builds of the library: the same bits, and the same time on the benchmark and the dense geometry.

  compare_forward_builds.py --parent DIR [--rounds 5] [--out profiles/forward_math_parent_vs_new.json]

DIR holds libfimex_amd.so and libfimex_amd_tuning.so built from the commit to compare with; the other side is this tree's.  The driver
(compare_builds.py) alternates the sides, one fresh process per side and round, and stops at the first that does not end normally.
Bits (sha256 of the output bytes): all ten methods (130 cells per bucket: the eight that are no median) on the geometries of the
forward tests of tests/test_gpu_parity.py with a few slices each, int16 and uint8 slices through the stored-type kernel, and, in the
tuning build, the kernels the product does not choose for these plans (lane kernels with look-ahead, wave per bucket, medians by
broadcast ranks and by rank counting).  Time (and bits), 100 slices: configs[3] (workloads.ForwardLambert, as scripts/bench_forward.py
sets it up) and the 0.1-degree global source onto 1-degree
global (100 cells per bucket, scripts/run_case.py forwarddense_*), mean, median and max each.
"""
import argparse, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compare_builds  # beside this script

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
compare_builds.add_arguments(ap, os.path.join(ROOT, "profiles", "forward_math_parent_vs_new.json"))
args = ap.parse_args()

# (inX, inY, outX, outY), nz, density, special, seed of cases.forward_positions: test_forward_methods_match_oracle, _long_buckets_wave_path,
# _dense_mappings, _tiled_mappings, _sparse_mappings_and_short_median
POSITIONS = [((140, 110, 60, 50), 5, d, True, 11) for d in (0.3, 1.0, 9.0)] + [((400, 300, 36, 26), 3, 130.0, True, 21)] + \
            [(s, 5, d, False, 23) for s, d in (((240, 200, 40, 30), 1.2), ((240, 200, 40, 30), 7.0), ((300, 256, 64, 48), 3.0))] + \
            [(s, 7, d, sp, 31) for s, d, sp in (((400, 300, 37, 29), 1.5, False), ((300, 200, 50, 33), 1.0, True), ((512, 200, 130, 13), 1.6, False),
                                                ((333, 377, 32, 80), 1.3, True), ((1203, 60, 60, 9), 1.8, False))] + \
            [(s, 9, d, True, 17) for s, d in (((150, 120, 64, 50), 0.08), ((150, 120, 63, 51), 0.08), ((300, 200, 100, 80), 0.5), ((200, 150, 40, 36), 2.5))]
EDGES = [((40, 28, 3, 2), 1), ((40, 28, 3, 2), 2), ((64, 48, 5, 70), 3), ((40, 30, 4, 3), 1300), ((257, 129, 33, 17), 37)]  # test_forward_tiled_edges
SWITCHES = [{"FWD_TILED": "0"}, {"FWD_TILED": "0", "FWD_WAVE": "1"}, {"FWD_MEDIAN_WAVE_MIN": "1", "FWD_MEDIAN_SELECT": "0"}, {"FWD_MEDIAN_WAVE": "0"},
            {"FWD_MEDIAN_SHORT": "0"}, {"FWD_TILED_SLOTS": "3"}, {"FWD_TILE_W": "8"}]


def worker():
    t_start = time.perf_counter()
    import numpy as np
    import torch
    from fimex_amd import capi as fa
    import workloads, bench
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    if args.lib:
        fa.LIB_PATH = os.path.join(args.lib, "libfimex_amd.so")
        fa.TUNING_LIB_PATH = os.path.join(args.lib, "libfimex_amd_tuning.so")
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    methods = list(range(fa.FORWARD_SUM, fa.FORWARD_SUM + 10))

    def report(case):  # "t": seconds since the worker started, for the record only
        print(json.dumps(dict(case, t=round(time.perf_counter() - t_start, 2))), flush=True)

    def sha(a):
        return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

    def field(nz, inY, inX, seed):
        f = cases.field(nz, inY, inX, seed=seed, nan_frac=0.03)
        f[:, ::3, ::2] = np.float32(0.0)
        f[:, 1::3, 1::2] = np.float32(-0.0)
        f[:, 2::7, ::3] = np.float32(281.5)
        f[:, 5::11, :] = np.nan
        return f

    def all_methods(name, px, py, f, shape, density=0.0):
        # 130 cells per bucket: without the medians, as test_forward_long_buckets_wave_path (some buckets are beyond the wave kernels' 256 cells)
        for m in (methods if density != 130.0 else [m for m in methods if m not in (fa.FORWARD_MEDIAN, fa.FORWARD_UNDEF_MEDIAN)]):
            report({"case": "%s method %d" % (name, m), "sha256": sha(fa.RegridPlan(m, px, py, *shape).apply_host(f))})

    for shape, nz, density, special, seed in POSITIONS:
        px, py = cases.forward_positions(*shape, seed=seed, density=density, special=special)
        all_methods("%dx%d_to_%dx%d density %g" % (shape + (density,)), px, py, field(nz, shape[1], shape[0], seed), shape, density)
    for shape, nz in EDGES:
        inX, inY, outX, outY = shape
        j, i = np.meshgrid(np.arange(inY, dtype=np.float64), np.arange(inX, dtype=np.float64), indexing="ij")
        px = ((i + 0.5) * outX / inX - 0.5 + 0.2 * np.sin(j / 7.0)).ravel()
        py = ((j + 0.5) * outY / inY - 0.5 + 0.2 * np.cos(i / 5.0)).ravel()
        f = cases.field(nz, inY, inX, seed=90, nan_frac=0.04)
        for k, v in enumerate((np.nan, 0.0, -0.0, np.inf, -np.inf)):
            if k < nz:
                f[(k * 7) % nz] = np.float32(v)
        all_methods("edges %dx%d_to_%dx%d nz %d" % (shape + (nz,)), px, py, f, shape)
    for shape, special in (((400, 300, 37, 29), False), ((300, 200, 50, 33), True)):  # stored types: staged tiles, and tiles read from memory
        px, py = cases.forward_positions(*shape, seed=41, density=1.5 if not special else 1.0, special=special)
        for dt, bad, code in ((np.int16, -32767.0, fa.CDM_SHORT), (np.uint8, 255.0, fa.CDM_UCHAR)):
            rng = np.random.default_rng(5)
            f = rng.integers(max(np.iinfo(dt).min, -3000) // 2, min(np.iinfo(dt).max, 3000) // 2 + 1, (3, shape[1], shape[0])).astype(dt)
            f.reshape(-1)[rng.choice(f.size, f.size // 20, replace=False)] = dt(bad)
            t = torch.from_numpy(f.view(np.uint8)).cuda()
            for m in methods:
                out = torch.zeros(3 * shape[2] * shape[3] * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
                fa.regrid_apply_typed_device(fa.RegridPlan(m, px, py, *shape), t.data_ptr(), code, 3, bad, out.data_ptr())
                torch.cuda.synchronize()
                report({"case": "%s %dx%d special %s method %d" % (np.dtype(dt).name, shape[0], shape[1], special, m), "sha256": sha(out.cpu().numpy())})

    fw = workloads.ForwardLambert()
    nz = 100
    d_in = bench.make_slices(torch, fw.base_field(), nz)

    def timed(name, plan, outY, outX):
        d_out = torch.empty((nz, outY, outX), dtype=torch.float32, device="cuda")
        ts = []
        for _ in range(7):  # two to warm up
            torch.cuda.synchronize()
            t0 = time.perf_counter(); plan.apply_device(d_in.data_ptr(), nz, d_out.data_ptr(), st); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        report({"case": name, "seconds": ts[2:], "sha256": sha(d_out.cpu().numpy())})

    x, y = fw.source_in_target_metres()
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    fa.points2position_device(dx.data_ptr(), dx.numel(), fw.x_axis, fa.PROJ_AXIS, st)
    fa.points2position_device(dy.data_ptr(), dy.numel(), fw.y_axis, fa.PROJ_AXIS, st)
    lon, lat = np.meshgrid(fw.src_lon, fw.src_lat)  # onto 1-degree global: scripts/run_case.py forwarddense_*
    px = workloads.axis_positions_numpy(lon.ravel(), np.arange(360) + 0.5 - 180.0); py = workloads.axis_positions_numpy(lat.ravel(), np.arange(180) + 0.5 - 90.0)
    for name, m in (("mean", fa.FORWARD_MEAN), ("median", fa.FORWARD_MEDIAN), ("max", fa.FORWARD_MAX)):
        timed("time_configs3_100_slices " + name, fa.RegridPlan.from_device(m, dx.data_ptr(), dy.data_ptr(), dx.numel(), fw.inX, fw.inY, fw.outX, fw.outY, st),
              fw.outY, fw.outX)
        timed("time_dense_100_cells_per_bucket_100_slices " + name, fa.RegridPlan(m, px, py, fw.inX, fw.inY, 360, 180), 180, 360)
    del d_in

    fa.use_tuning_build(True)  # the kernels behind the switches, on one dense and one sparse geometry
    for shape, density, seed in (((240, 200, 40, 30), 7.0, 23), ((400, 300, 36, 26), 130.0, 21), ((200, 150, 40, 36), 2.5, 17)):
        px, py = cases.forward_positions(*shape, seed=seed, density=density, special=False)
        f = field(5, shape[1], shape[0], seed)
        for sw in SWITCHES:
            for k, v in sw.items():
                os.environ["FIMEX_AMD_" + k] = v
            all_methods("tuning %s %dx%d density %g" % (",".join("%s=%s" % kv for kv in sw.items()), shape[0], shape[1], density), px, py, f, shape, density)
            for k in sw:
                del os.environ["FIMEX_AMD_" + k]


WHAT = ("The forward regrid: bits of all ten methods on the geometries of the forward tests, on int16 and uint8 slices and, in the tuning build, "
        "through the kernels behind the FWD_* switches; time of apply_device on 100 slices of configs[3] and of the 0.1-degree global source onto "
        "1-degree global (100 cells per bucket), mean, median and max (host clock around the call and a device synchronisation).")

worker() if args.worker else compare_builds.drive(__file__, args, WHAT)
