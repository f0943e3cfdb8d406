#!/usr/bin/env python3
"""Vertical interpolation plans on the workload of scripts/bench_vertical.py: 65 model levels to 20 pressure levels on 2000 x 2000,
method log, 5 % NaN, nt = 1, input levels as HYBRID_SIGMA_AP and as an explicit FIELD.  Device-resident, HIP-event timed, median of
--launches calls after 3 warm-up calls.  Per kind of input levels it times
  the one-shot call fimex_amd_vertical_interpolate_device (search and data in one kernel, per variable),
  the build of a plan (fimex_amd_vertical_plan_create_device: allocation of the entries and the search),
  the apply for float and for packed short variables, 1 and 6 of them per call,
and, as the yardstick of each, a device-to-device copy that moves the same number of bytes (half read, half written) in the same
run.  Algorithmic bytes of an apply: the entries (8 bytes per output cell), the outputs, and per variable min(nzi, 2 nzo) input
planes.  It reports apply / copy, apply / one-shot per variable and the break-even number of variables,
build / (one-shot - apply).  The results of the timed calls are compared at this size: the float apply with the one-shot call bit for
bit, the short apply with the chain data2interpolation -> one-shot -> interpolation2data byte for byte.
Writes profiles/vertical_plan.json (or --out) and prints one JSON line per measurement.
usage: python scripts/bench_vertical_plan.py [--kinds ap,field] [--launches 20] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_others import timed
from bench_vertical import NX, NY, NZI, NZO, LEVEL1, hybrid_coefficients

NVARS = (1, 6)
SHORT_FILL = -32768


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--kinds", default="ap,field")
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical_plan.json"))
    args = ap_.parse_args()
    import torch
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    plane, nt, nmax = NX * NY, 1, max(NVARS)
    ap, b = hybrid_coefficients()
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    jj = torch.arange(NY, device="cuda", dtype=torch.float32)[:, None]
    ii = torch.arange(NX, device="cuda", dtype=torch.float32)[None, :]
    terrain = 0.5 + 0.5 * torch.sin(0.011 * ii) * torch.cos(0.007 * jj)  # surface pressure from 600 (mountains) to 1040 hPa
    ps = (600. + 440. * terrain + 3. * torch.randn((NY, NX), device="cuda", generator=gen))[None].contiguous()
    # six variables of their own: nothing is read twice because two variables share memory
    floats, shorts = [], []
    for v in range(nmax):
        d = 280. + torch.randn((nt, NZI, NY, NX), device="cuda", generator=gen)
        nan = torch.rand((nt, NZI, NY, NX), device="cuda", generator=gen) < 0.05
        s = torch.round((d - 280.) * 500.).to(torch.int16)
        d[nan] = float("nan")
        s[nan] = SHORT_FILL
        floats.append(d); shorts.append(s)
        del nan
    fouts = [torch.empty((nt, NZO, NY, NX), dtype=torch.float32, device="cuda") for _ in range(nmax)]
    souts = [torch.empty((nt, NZO, NY, NX), dtype=torch.int16, device="cuda") for _ in range(nmax)]
    one = torch.empty((nt, NZO, NY, NX), dtype=torch.float32, device="cuda")
    hybrid = fa.VerticalLevels.hybrid_sigma_ap(ap, b, ps.data_ptr())
    cells_in, cells_out = nt * NZI * plane, nt * NZO * plane

    def copy_of(nbytes):
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        ms, mn = timed(torch, lambda: dst.copy_(src), reps=args.launches, warm=3)
        return ms, mn

    results = []

    def record(r):
        r["device"] = torch.cuda.get_device_name(0)
        r["launches"] = args.launches
        print(json.dumps(r), flush=True)
        results.append(r)

    for kind in args.kinds.split(","):
        name = "HYBRID_SIGMA_AP" if kind == "ap" else "FIELD"
        case = "%d -> %d levels, %d x %d, nt = %d, method log, input levels %s" % (NZI, NZO, NX, NY, nt, name)
        if kind == "field":
            field = torch.empty((nt, NZI, NY, NX), dtype=torch.float32, device="cuda")
            fa.vertical_levels_device(hybrid, NX, NY, nt, field.data_ptr(), st)
            levels = fa.VerticalLevels.from_field(field.data_ptr(), NZI)
            level_bytes = 4 * cells_in
        else:
            field, levels, level_bytes = None, hybrid, 4 * nt * plane
        # the one-shot call: the parent's code path, per variable
        alg = 4 * (cells_in + cells_out) + level_bytes
        copy_ms, copy_min = copy_of(alg)
        ms, mn = timed(torch, lambda: fa.vertical_interpolate_device(fa.VINT_METHOD_LOG, NX, NY, nt, floats[0].data_ptr(), levels, one.data_ptr(),
                                                                      level1=LEVEL1, stream=st), reps=args.launches, warm=3)
        one_ms = ms
        record({"case": case, "what": "one-shot call, one float variable", "ms_median": ms, "ms_min": mn, "algorithmic_bytes": alg,
                "TBps": alg / ms / 1e9, "copy_ms_median": copy_ms, "copy_ms_min": copy_min, "over_copy": ms / copy_ms})
        # the build: the plan's entries are allocated and filled by every call
        alg = 8 * cells_out + level_bytes
        copy_ms, copy_min = copy_of(alg)
        ms, mn = timed(torch, lambda: fa.VerticalPlan(fa.VINT_METHOD_LOG, NX, NY, nt, levels, None, LEVEL1, device=True, stream=st).close(),
                       reps=args.launches, warm=3)
        build_ms = ms
        record({"case": case, "what": "plan build (allocation and search)", "ms_median": ms, "ms_min": mn, "algorithmic_bytes": alg,
                "TBps": alg / ms / 1e9, "copy_ms_median": copy_ms, "copy_ms_min": copy_min, "over_copy": ms / copy_ms})
        plan = fa.VerticalPlan(fa.VINT_METHOD_LOG, NX, NY, nt, levels, None, LEVEL1, device=True, stream=st)
        first, second, _ = plan.entries()
        defined = float(np.mean(first != second))
        # neighbouring cells that share both levels: what lets a lane fetch 16 bytes per side
        shared = float(np.mean((first[..., 1:] == first[..., :-1]) & (second[..., 1:] == second[..., :-1])))
        del first, second
        apply_ms = {}
        for label, ins, outs, code, elem, fill in (("float", floats, fouts, fa.CDM_FLOAT, 4, float("nan")), ("short", shorts, souts, fa.CDM_SHORT, 2, SHORT_FILL)):
            for nvar in NVARS:
                alg = 8 * cells_out + nvar * elem * (cells_out + nt * plane * min(NZI, 2 * NZO))
                copy_ms, copy_min = copy_of(alg)
                pin, pout = [t.data_ptr() for t in ins[:nvar]], [t.data_ptr() for t in outs[:nvar]]
                ms, mn = timed(torch, lambda: plan.apply_device(pin, code, pout, badValue=fill, stream=st), reps=args.launches, warm=3)
                apply_ms[(label, nvar)] = ms
                record({"case": case, "what": "apply, %d %s variable%s" % (nvar, label, "s" if nvar > 1 else ""), "nvar": nvar, "ms_median": ms,
                        "ms_min": mn, "ms_per_variable": ms / nvar, "algorithmic_bytes": alg, "TBps": alg / ms / 1e9, "copy_ms_median": copy_ms,
                        "copy_ms_min": copy_min, "over_copy": ms / copy_ms, "per_variable_over_one_shot": ms / nvar / one_ms})
        # the results of what was timed
        torch.cuda.synchronize()
        same = ((fouts[0].view(torch.int32) == one.view(torch.int32)) | (torch.isnan(fouts[0]) & torch.isnan(one))).all().item()
        tmp = torch.empty_like(floats[0])
        fa.data2interpolation_device(shorts[0].data_ptr(), fa.CDM_SHORT, cells_in, SHORT_FILL, tmp.data_ptr(), st)
        fa.vertical_interpolate_device(fa.VINT_METHOD_LOG, NX, NY, nt, tmp.data_ptr(), levels, one.data_ptr(), level1=LEVEL1, stream=st)
        chain = torch.empty_like(souts[0])
        fa.interpolation2data_device(one.data_ptr(), cells_out, fa.CDM_SHORT, SHORT_FILL, chain.data_ptr(), st)
        torch.cuda.synchronize()
        same_short = torch.equal(chain, souts[0])
        del tmp, chain
        a1 = apply_ms[("float", 1)]
        record({"case": case, "what": "summary", "one_shot_ms": one_ms, "build_ms": build_ms, "apply_float_ms": a1,
                "apply_float_6_ms_per_variable": apply_ms[("float", 6)] / 6, "apply_short_ms": apply_ms[("short", 1)],
                "apply_short_6_ms_per_variable": apply_ms[("short", 6)] / 6, "one_shot_over_apply_float": one_ms / a1,
                "break_even_variables": build_ms / (one_ms - a1) if one_ms > a1 else None,
                "break_even_variables_6_per_call": build_ms / (one_ms - apply_ms[("float", 6)] / 6) if one_ms > apply_ms[("float", 6)] / 6 else None,
                "defined_share_of_entries": defined, "x_neighbours_sharing_both_levels": shared,
                "float_apply_equals_one_shot": bool(same), "short_apply_equals_chain": bool(same_short)})
        assert same and same_short, "the plan's results differ from the one-shot call's"
        plan.close()
        del field
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"script": "scripts/bench_vertical_plan.py",
                   "timing": "HIP events around one call, median of the launches after 3 warm-up calls; copies of the same bytes in the same run",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
