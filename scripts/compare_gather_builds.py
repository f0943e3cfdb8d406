#!/usr/bin/env python3
"""Compares the per-lane gather regrid and the fused merger of two builds of the library: the same bits, and the same time.

  compare_gather_builds.py --parent DIR [--rounds 5] [--out profiles/gather_entry_parent_vs_new.json]

DIR holds libfimex_amd.so and libfimex_amd_tuning.so built from the commit to compare with; the other side is this tree's.  The driver
(compare_builds.py) alternates the sides, one fresh process per side and round, and stops at the first that does not end normally.
Bits (sha256 of the output bytes): apply_gather_device, three methods, on the geometries of test_gather_and_lds_staged_paths_agree_with_oracle
(tests/test_gpu_parity.py) with the test's slice count and with 1, 2 and 3 slices; in the tuning build one slice with 4 and 8 cells per lane
and the stored-type gather, five types x three methods, with the switches of test_typed_gather_main_loops_with_forced_chunks
(tests/test_gpu_z_chunks.py); the fused merger on the cases of tests/test_gpu_merge.py.  Time (and bits): the benchmark geometry
(workloads.BilinearRotatedPole), 200 slices through apply_gather_device, three methods; bilinear and nearest one slice per call on a
different slice pair every call (bench.py's single_slice_cold; per pass over the ring the mean of the calls counts as one launch);
bilinear on 3 slices; int32 bilinear on 200 slices through regrid_apply_typed_device; the fused merger as scripts/bench_merge.py sets it up.
"""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compare_builds  # beside this script

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
compare_builds.add_arguments(ap, os.path.join(ROOT, "profiles", "gather_entry_parent_vs_new.json"))
args = ap.parse_args()

SHAPES = [(400, 300, 200, 200, 10), (1000, 700, 333, 257, 7), (128, 96, 640, 480, 3), (64, 2000, 50, 300, 5)]  # inX, inY, outX, outY, nz
TYPED_GEOMETRY, TYPED_NZ = (97, 71, 151, 110), 19
TYPED = [("int16", -32767.0), ("uint16", 65535.0), ("int8", -127.0), ("uint8", 255.0), ("int32", -2147483647.0)]


def worker():
    import numpy as np
    import torch
    from fimex_amd import capi as fa
    import workloads, bench
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import cases, oracle
    import test_gpu_merge as tm
    import bench_merge as bm
    import merge_ref as mr
    if args.lib:
        fa.LIB_PATH = os.path.join(args.lib, "libfimex_amd.so")
        fa.TUNING_LIB_PATH = os.path.join(args.lib, "libfimex_amd_tuning.so")
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    methods = (("nearest", fa.NEAREST_NEIGHBOR), ("bilinear", fa.BILINEAR), ("bicubic", fa.BICUBIC))

    def sha(t):
        return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()

    def report(name, t, seconds=None):
        print(json.dumps(dict({"case": name, "sha256": sha(t)}, **({"seconds": seconds} if seconds else {}))), flush=True)

    def gather_bits(tag):
        for inX, inY, outX, outY, nz in SHAPES:
            px, py = cases.backward_positions(inX, inY, outX, outY, seed=inX + outX)
            d_in = torch.from_numpy(cases.field(nz, inY, inX, seed=3)).cuda()
            for name, m in methods:
                plan = fa.RegridPlan(m, px, py, inX, inY, outX, outY)
                for n in sorted({1, 2, 3, nz}):
                    d_out = torch.full((n, outY, outX), -7.0, dtype=torch.float32, device="cuda")
                    plan.apply_gather_device(d_in.data_ptr(), n, d_out.data_ptr(), st)
                    torch.cuda.synchronize()
                    report("%sgather %s %dx%d_to_%dx%d nz %d" % (tag, name, inX, inY, outX, outY, n), d_out)
                if tag:
                    break  # the tuning switches below change the one-slice kernel only

    gather_bits("")
    for geometry, smooth_method, method, nz, use_outer in tm.MERGE_CASES:
        inner, outer, target = tm.GEOMETRIES[geometry]
        I, O = tm._merge_fields(geometry, nz)
        plan, keep = tm._plans(fa, geometry, smooth_method, method, 5, 2, use_outer)
        dI, dO = torch.from_numpy(np.array(I)).cuda(), torch.from_numpy(np.array(O)).cuda()
        fused = torch.full((nz,) + target.shape, -7.0, dtype=torch.float32, device="cuda")
        plan.apply_device(dI.data_ptr(), dO.data_ptr(), nz, fused.data_ptr(), st)
        torch.cuda.synchronize()
        report("merge %s step1 %d steps34 %d nz %d useOuter %d" % (geometry, smooth_method, method, nz, use_outer), fused)
        plan.close()

    def timed(name, launch, d_out, warm=2, reps=3):
        for _ in range(warm): launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); launch(); b.record()
            torch.cuda.synchronize(); ts.append(a.elapsed_time(b) / 1e3)
        report(name, d_out, ts)

    wl = workloads.BilinearRotatedPole()
    NZ = 200
    d_f = bench.make_slices(torch, wl.base_field(), NZ)
    d_out = torch.empty((NZ, wl.outY, wl.outX), dtype=torch.float32, device="cuda")
    in_layer, out_layer = wl.inX * wl.inY, wl.outX * wl.outY
    ring = [(k * 7) % NZ for k in range(60)]
    for name, m in methods:
        plan, _, _ = bench.build_plan(fa, torch, wl, m, st)
        timed("time_gather_%s_nz200" % name, lambda: plan.apply_gather_device(d_f.data_ptr(), NZ, d_out.data_ptr(), st), d_out)
        if name == "bicubic":
            continue
        if name == "bilinear":
            timed("time_gather_bilinear_nz3", lambda: plan.apply_gather_device(d_f.data_ptr(), 3, d_out.data_ptr(), st), d_out[:3], warm=5, reps=10)
        d_out.zero_()
        means = []
        for rep in range(4):  # the first pass warms up
            it = iter(ring)

            def one_cold():
                k = next(it)
                plan.apply_gather_device(d_f.data_ptr() + 4 * in_layer * k, 1, d_out.data_ptr() + 4 * out_layer * k, st)
            _, ms = bench.time_launches(torch, one_cold, len(ring), 0, False)
            means.append(float(np.mean(ms)) / 1e3)
        report("time_gather_%s_one_slice_cold" % name, d_out[sorted(ring)], means[1:])
    d_i32 = torch.nan_to_num(d_f * 100, nan=-2147483647.0).to(torch.int32)
    del d_f
    d_out32 = d_out.view(torch.int32)
    plan, _, _ = bench.build_plan(fa, torch, wl, fa.BILINEAR, st)
    timed("time_typed_int32_bilinear_nz200", lambda: fa.regrid_apply_typed_device(plan, d_i32.data_ptr(), fa.CDM_INT, NZ, -2147483647.0, d_out32.data_ptr(), st), d_out32)
    del d_i32, d_out, d_out32, plan
    torch.cuda.empty_cache()

    nz = 65  # scripts/bench_merge.py
    ox, oy = bm.STEP_O * np.arange(bm.OUTER[0]), bm.STEP_O * np.arange(bm.OUTER[1])
    i0 = ((ox[-1] - (bm.INNER[0] - 1)) / 2, (oy[-1] - (bm.INNER[1] - 1)) / 2)
    ix, iy = i0[0] + np.arange(bm.INNER[0]), i0[1] + np.arange(bm.INNER[1])
    tx, ty = mr.extend_inner_axis(ix, ox), mr.extend_inner_axis(iy, oy)
    oi = fa.RegridPlan(fa.BILINEAR, *bm.index_positions((0., 0.), bm.STEP_O, ix, iy), bm.OUTER[0], bm.OUTER[1], bm.INNER[0], bm.INNER[1])
    it = fa.RegridPlan(fa.BILINEAR, *bm.index_positions(i0, 1.0, tx, ty), bm.INNER[0], bm.INNER[1], tx.size, ty.size)
    ot = fa.RegridPlan(fa.BILINEAR, *bm.index_positions((0., 0.), bm.STEP_O, tx, ty), bm.OUTER[0], bm.OUTER[1], tx.size, ty.size)
    merge = fa.MergePlan(oi, it, ot, 5, 2, True)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)

    def field(nx, ny, x0, y0, step):
        jj = (y0 + step * torch.arange(ny, dtype=torch.float32, device="cuda"))[None, :, None]
        ii = (x0 + step * torch.arange(nx, dtype=torch.float32, device="cuda"))[None, None, :]
        zz = torch.arange(nz, dtype=torch.float32, device="cuda")[:, None, None]
        return (280. + 8. * torch.sin(0.004 * ii + 0.1 * zz) * torch.cos(0.005 * jj) + 0.3 * torch.randn((nz, ny, nx), device="cuda", generator=gen)).contiguous()

    I = field(bm.INNER[0], bm.INNER[1], i0[0], i0[1], 1.0)
    I[torch.rand(I.shape, device="cuda", generator=gen) < 0.01] = float("nan")
    O = field(bm.OUTER[0], bm.OUTER[1], 0., 0., bm.STEP_O)
    fused = torch.full((nz, ty.size, tx.size), -1.0, dtype=torch.float32, device="cuda")
    timed("time_merge_fused_bilinear_nz65", lambda: merge.apply_device(I.data_ptr(), O.data_ptr(), nz, fused.data_ptr(), st), fused)
    del I, O, fused
    torch.cuda.empty_cache()

    fa.use_tuning_build(True)
    for cells in ("4", "8"):
        os.environ["FIMEX_AMD_FEW_CELLS"] = cells
        gather_bits("tuning FEW_CELLS=%s " % cells)
    del os.environ["FIMEX_AMD_FEW_CELLS"]
    os.environ["FIMEX_AMD_TYPED_STAGED"], os.environ["FIMEX_AMD_TYPED_FUSED"] = "0", "2"
    inX, inY, outX, outY = TYPED_GEOMETRY
    px, py = cases.backward_positions(inX, inY, outX, outY, seed=12)
    for dtname, bad in TYPED:
        dt = np.dtype(dtname).type
        rng, info = np.random.default_rng(3), np.iinfo(dt)
        f = rng.integers(max(info.min, -30000) // 2, min(info.max, 30000) // 2 + 1, (TYPED_NZ, inY, inX)).astype(dt)
        f.reshape(-1)[rng.choice(f.size, f.size // 25, replace=False)] = dt(bad)
        t = torch.from_numpy(f.view(np.uint8)).cuda()
        for name, m in methods:
            plan = fa.RegridPlan(m, px, py, inX, inY, outX, outY)
            for zpb in ("8", "17"):
                os.environ["FIMEX_AMD_ZPB"] = zpb
                out = torch.full((TYPED_NZ * outY * outX * np.dtype(dt).itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
                fa.regrid_apply_typed_device(plan, t.data_ptr(), oracle.cdm_type_of(dt), TYPED_NZ, bad, out.data_ptr(), st)
                torch.cuda.synchronize()
                report("tuning typed gather %s %s ZPB=%s" % (dtname, name, zpb), out)


WHAT = ("The per-lane gather regrid (float slices and stored types) and the fused merger: bits on the geometries of the tests, time of the "
        "launches on the benchmark geometry and on the merger's benchmark (HIP events around each launch).")

worker() if args.worker else compare_builds.drive(__file__, args, WHAT)
