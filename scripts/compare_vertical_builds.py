#!/usr/bin/env python3
"""Compares the vertical, time and 1-D blend kernels of two builds of the library: the same bits, and the same time.

  compare_vertical_builds.py --parent DIR [--rounds 5] [--out profiles/vertical_blend_parent_vs_new.json]

DIR holds libfimex_amd.so and libfimex_amd_tuning.so built from the commit to compare with; the other side is this tree's pair.  The
driver (compare_builds.py) alternates the sides, one fresh process per side and round, and stops at the first that does not end
normally.
Bits (sha256 of the output bytes), on the small shapes of the GPU tests, product and tuning build: every vertical method on every
input level kind, fixed and template levels (tests/test_gpu_vertical.py: make_case) through the one-shot entry, the plan's entries
and its float apply; the plan's apply on packed shorts; every column walked and groups of 8 (tuning build); the seven 1-D blends on
each branch, the double blend; the time interpolation of every stored type on the axes of tests/time_quality_ref.py.
Time (and bits): the nt = 1 cases of scripts/bench_vertical.py (65 hybrid -> 20 pressure levels on 2000 x 2000, method log), the plan
build and the float and short applies of scripts/bench_vertical_plan.py, the float case of scripts/bench_time_quality.py, and one
get_values_1d_f_device blend of 4 M floats.
"""
import argparse, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compare_builds  # beside this script

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
compare_builds.add_arguments(ap, os.path.join(ROOT, "profiles", "vertical_blend_parent_vs_new.json"))
args = ap.parse_args()


def worker():
    import numpy as np
    import torch
    from fimex_amd import capi as fa
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_vertical as tgv
    import time_quality_ref as tq
    import vertical_ref as vr
    from bench_vertical import NX, NY, NZI, NZO, LEVEL1, hybrid_coefficients
    if args.lib:
        fa.LIB_PATH = os.path.join(args.lib, "libfimex_amd.so")
        fa.TUNING_LIB_PATH = os.path.join(args.lib, "libfimex_amd_tuning.so")
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    def bits(name, *arrays):
        print(json.dumps({"case": name, "sha256": sha(*arrays)}), flush=True)

    # ---- bits: the vertical kernels
    small = tgv.CONFIGS[:6]
    made = {}

    def case(method, kind_in, template):
        i = method * 10 + kind_in * 2 + int(template)
        if i not in made:
            nx, ny, nt, nzi, nzo, order = small[i % len(small)]
            kind_out = vr.KINDS[(kind_in + 1 + method) % 5] if template else None
            made[i] = tgv.make_case(1000 + i, kind_in, kind_out, nx, ny, nt, nzi, nzo, order, method in (vr.LOG, vr.LOGLOG))
        return made[i]

    def vertical(build, method, kind_in, template):
        data, inL, outL, level1 = case(method, kind_in, template)
        nt, _, ny, nx = data.shape
        li, lo = tgv._fa_levels(fa, inL), tgv._fa_levels(fa, outL) if outL is not None else None
        one = fa.vertical_interpolate_host(method, data, li, lo, level1)
        plan = fa.VerticalPlan(method, nx, ny, nt, li, lo, level1)
        first, second, factor = plan.entries()
        applied = plan.apply_host(data)
        with np.errstate(invalid="ignore"):
            packed = np.where(np.isnan(data), -32768, np.clip(np.round((data - 280.0) * 100), -32000, 32000)).astype(np.int16)
        shorts = plan.apply_host(packed, badValue=-32768.0)
        plan.close()
        bits("%s method %d kind %d %s" % (build, method, kind_in, "template" if template else "fixed"), one, first, second, factor, applied, shorts)

    for tuning in (False, True):
        fa.use_tuning_build(tuning)
        build = "tuning" if tuning else "product"
        for method in vr.METHODS:
            for kind_in in vr.KINDS:
                for template in (False, True):
                    vertical(build, method, kind_in, template)
    for bisect, group in ((0, 4), (1, 8), (0, 8)):  # still the tuning build
        os.environ["FIMEX_AMD_VERTICAL_BISECT"], os.environ["FIMEX_AMD_VERTICAL_GROUP"] = str(bisect), str(group)
        for kind_in in (vr.FIELD, vr.HYBRID_SIGMA):
            vertical("tuning bisect %d group %d" % (bisect, group), vr.LIN, kind_in, False)
            vertical("tuning bisect %d group %d" % (bisect, group), vr.LOG, kind_in, True)
    del os.environ["FIMEX_AMD_VERTICAL_BISECT"], os.environ["FIMEX_AMD_VERTICAL_GROUP"]

    # ---- bits: the 1-D blends and the time interpolation
    rng = np.random.default_rng(7)
    A, B = rng.normal(280, 5, 1961).astype(np.float32), rng.normal(275, 5, 1961).astype(np.float32)
    A[::17], B[5::19] = np.nan, np.nan
    for tuning in (False, True):
        fa.use_tuning_build(tuning)
        build = "tuning" if tuning else "product"
        for kind in range(7):
            outs = [fa.get_values_1d_host(kind, A, B, a, b, x) for a, b, x in ((2., 5., 3.), (2., 5., 2.), (2., 5., 5.), (2., 5., 20.), (5., 2., 5.5), (3., 3., 1.))]
            bits("%s blend kind %d" % (build, kind), *outs)
        dA, dB = torch.from_numpy(A.astype(np.float64)).cuda(), torch.from_numpy(B.astype(np.float64)).cuda()
        dout = torch.empty_like(dA)
        outs = []
        for a, b, x in ((2., 5., 3.), (2., 5., 2.), (2., 5., 5.), (2., 5., 20.)):
            fa.get_values_linear_d_device(dA.data_ptr(), dB.data_ptr(), dout.data_ptr(), A.size, a, b, x)
            torch.cuda.synchronize()
            outs.append(dout.cpu().numpy())
        bits("%s blend of doubles" % build, *outs)
        for axis in sorted(tq.AXES):
            old, new = tq.AXES[axis]
            outs = [fa.time_interpolate_host(tq.series(100 + code, tq.DTYPES[code], old.size, n), old, new) for code in tq.TYPES for n in (63, 260)]
            bits("%s time axis %s" % (build, axis), *outs)
        old = np.arange(10.0)  # 300 steps: more than a launch, chunk boundaries inside runs
        new = np.concatenate([np.linspace(0.005, 1.0, 100), np.linspace(1.005, 2.0, 100), np.linspace(2.01, 3.0, 56), np.linspace(3.01, 9.9, 44)])
        bits("%s time 300 steps" % build, fa.time_interpolate_host(tq.series(300, np.int16, old.size, 68), old, new),
             fa.time_interpolate_host(tq.series(301, np.float32, old.size, 5000), old, new))
    fa.use_tuning_build(False)

    # ---- time (and bits)
    def timed(name, launch, result, reps=8, warm=3):
        ts = []
        for i in range(warm + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); launch(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        print(json.dumps({"case": name, "seconds": ts[warm:], "sha256": sha(*result())}), flush=True)

    plane, nt = NX * NY, 1
    cap, cb = hybrid_coefficients()
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    jj = torch.arange(NY, device="cuda", dtype=torch.float32)[:, None]
    ii = torch.arange(NX, device="cuda", dtype=torch.float32)[None, :]
    terrain = 0.5 + 0.5 * torch.sin(0.011 * ii) * torch.cos(0.007 * jj)
    ps = (600. + 440. * terrain + 3. * torch.randn((NY, NX), device="cuda", generator=gen))[None].contiguous()
    data = 280. + torch.randn((nt, NZI, NY, NX), device="cuda", generator=gen)
    nan = torch.rand((nt, NZI, NY, NX), device="cuda", generator=gen) < 0.05
    shorts = torch.round((data - 280.) * 500.).to(torch.int16)
    data[nan] = float("nan")
    shorts[nan] = -32768
    del nan
    out = torch.empty((nt, NZO, NY, NX), dtype=torch.float32, device="cuda")
    sout = torch.empty((nt, NZO, NY, NX), dtype=torch.int16, device="cuda")
    hybrid = fa.VerticalLevels.hybrid_sigma_ap(cap, cb, ps.data_ptr())
    field = torch.empty((nt, NZI, NY, NX), dtype=torch.float32, device="cuda")
    fa.vertical_levels_device(hybrid, NX, NY, nt, field.data_ptr(), st)
    for name, levels in (("HYBRID_SIGMA_AP", hybrid), ("FIELD", fa.VerticalLevels.from_field(field.data_ptr(), NZI))):
        timed("time_vertical_65to20_log_%s" % name,
              lambda: fa.vertical_interpolate_device(fa.VINT_METHOD_LOG, NX, NY, nt, data.data_ptr(), levels, out.data_ptr(), level1=LEVEL1, stream=st),
              lambda: [out.cpu().numpy()])
        plans = []

        def build():
            while plans:
                plans.pop().close()
            plans.append(fa.VerticalPlan(fa.VINT_METHOD_LOG, NX, NY, nt, levels, None, LEVEL1, device=True, stream=st))
        timed("time_plan_build_%s" % name, build, lambda: plans[0].entries())
        plan = plans.pop()
        timed("time_plan_apply_float_%s" % name, lambda: plan.apply_device(data.data_ptr(), fa.CDM_FLOAT, out.data_ptr(), stream=st), lambda: [out.cpu().numpy()])
        timed("time_plan_apply_short_%s" % name, lambda: plan.apply_device(shorts.data_ptr(), fa.CDM_SHORT, sout.data_ptr(), badValue=-32768, stream=st),
              lambda: [sout.cpu().numpy()])
        plan.close()
    del data, shorts, out, sout, field, ps

    n = plane
    n_old, n_new = 25, 145  # scripts/bench_time_quality.py
    old, new = np.arange(n_old) * 3600.0, np.arange(n_new) * 600.0
    series = (280.0 + 10.0 * torch.randn((n_old, n), device="cuda", generator=gen)).contiguous()
    tout = torch.empty((n_new, n), dtype=torch.float32, device="cuda")
    timed("time_time_interpolate_float_25to145", lambda: fa.time_interpolate_device(series.data_ptr(), fa.CDM_FLOAT, n, old, new, tout.data_ptr(), stream=st),
          lambda: [tout[::12].cpu().numpy()])
    timed("time_blend_linear_4M", lambda: fa.get_values_1d_device(fa.BLEND_LINEAR, series[0].data_ptr(), series[1].data_ptr(), tout[0].data_ptr(), n,
                                                                  2., 5., 3., stream=st), lambda: [tout[0].cpu().numpy()])


WHAT = ("The vertical interpolation (one-shot kernel, plan build, plan apply), the time interpolation and the 1-D blends before and after the "
        "blends moved into blend_math.hpp and the host side of the level search into vertical_search.hpp: bits of every method and level kind on "
        "the shapes of the GPU tests, product and tuning build; time of the 65 -> 20 level case on 2000 x 2000 (method log) through the one-shot "
        "entry, the plan build and the float and short applies, of 25 -> 145 time steps on 4 M floats and of one 4 M blend (host clock around "
        "the call and a device synchronisation).")

worker() if args.worker else compare_builds.drive(__file__, args, WHAT, worker_timeout=400)
