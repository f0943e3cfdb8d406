#!/usr/bin/env python3
"""Grid merging on packed shorts (fimex_amd_merge_apply_typed_device) on the workload of scripts/bench_merge.py: 65 slices, a
2000 x 2000 inner grid centred in a 1000 x 750 outer grid of four times the step, the target the inner grid continued over the
outer one (3996 x 2996), bilinear on all three plans, LINEAR(5, 2), 1 % fill values in the inner.  Inner: short, scale 0.01,
offset 273.15, fill -32768; outer: short, scale 0.02, offset 250, fill -32767.

Three forms and a device copy alternate launch by launch in one process on the same buffers: the typed entry (`typed_fused`, the
two fused kernels on shorts), fimex_amd_merge_apply_typed_chain_device (`typed_chain`, regrid_apply_typed three times and the two
typed elementwise kernels on stored-type temporaries) and the float entry fimex_amd_merge_apply_device on float copies of the same
fields (`float_fused`).  Before timing, the typed entry's result is compared with the chain's byte for byte.  Per form: the median
of --reps timed calls after --warmup, HIP events around one call; the spread (max - min); bytes moved, counted from the code, and
TB/s on them.

usage: python scripts/bench_merge_typed.py [--reps 20] [--warmup 3] [--nz 65] [--out profiles/merge_typed.json]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INNER = (2000, 2000)   # nx, ny, step 1
OUTER = (1000, 750)    # nx, ny, step 4
STEP_O = 4.0
NAN = float("nan")


def index_positions(src0, src_step, dst_x, dst_y):
    """fractional (column, row) of the mesh of two target axes on a source grid with origin src0 and one step"""
    X, Y = np.meshgrid(dst_x, dst_y)
    return ((X - src0[0]) / src_step).ravel(), ((Y - src0[1]) / src_step).ravel()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nz", type=int, default=65)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_typed.json"))
    a = ap.parse_args()
    import torch
    import merge_ref as mr
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    nz = a.nz
    ox, oy = STEP_O * np.arange(OUTER[0]), STEP_O * np.arange(OUTER[1])
    i0 = ((ox[-1] - (INNER[0] - 1)) / 2, (oy[-1] - (INNER[1] - 1)) / 2)
    ix, iy = i0[0] + np.arange(INNER[0]), i0[1] + np.arange(INNER[1])
    tx, ty = mr.extend_inner_axis(ix, ox), mr.extend_inner_axis(iy, oy)
    oi = fa.RegridPlan(fa.BILINEAR, *index_positions((0., 0.), STEP_O, ix, iy), OUTER[0], OUTER[1], INNER[0], INNER[1])
    it = fa.RegridPlan(fa.BILINEAR, *index_positions(i0, 1.0, tx, ty), INNER[0], INNER[1], tx.size, ty.size)
    ot = fa.RegridPlan(fa.BILINEAR, *index_positions((0., 0.), STEP_O, tx, ty), OUTER[0], OUTER[1], tx.size, ty.size)
    plan = fa.MergePlan(oi, it, ot, 5, 2, True)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)

    def field(nx, ny, x0, y0, step):
        jj = (y0 + step * torch.arange(ny, dtype=torch.float32, device="cuda"))[None, :, None]
        ii = (x0 + step * torch.arange(nx, dtype=torch.float32, device="cuda"))[None, None, :]
        zz = torch.arange(nz, dtype=torch.float32, device="cuda")[:, None, None]
        return (280. + 8. * torch.sin(0.004 * ii + 0.1 * zz) * torch.cos(0.005 * jj) + 0.3 * torch.randn((nz, ny, nx), device="cuda", generator=gen)).contiguous()

    pI, pO = fa.Packing(fa.CDM_SHORT, -32768.0, 0.01, 273.15), fa.Packing(fa.CDM_SHORT, -32767.0, 0.02, 250.0)

    def packed(f, p):  # the field as a writer packs it, NaN as the fill value, and the float array a reader makes of that
        raw = torch.empty(f.shape, dtype=torch.int16, device="cuda")
        fa.convert_scaled_device(f.data_ptr(), fa.CDM_FLOAT, f.numel(), NAN, 1.0, 0.0, fa.CDM_SHORT, p.fill, p.scale, p.offset, raw.data_ptr(), st)
        fa.convert_scaled_device(raw.data_ptr(), fa.CDM_SHORT, f.numel(), p.fill, p.scale, p.offset, fa.CDM_FLOAT, NAN, 1.0, 0.0, f.data_ptr(), st)
        return raw, f

    I = field(INNER[0], INNER[1], i0[0], i0[1], 1.0)
    I[torch.rand(I.shape, device="cuda", generator=gen) < 0.01] = NAN
    rI, fI = packed(I, pI)
    rO, fO = packed(field(OUTER[0], OUTER[1], 0., 0., STEP_O), pO)
    shape = (nz, ty.size, tx.size)
    out_fused = torch.full(shape, -1, dtype=torch.int16, device="cuda")
    out_chain = torch.full(shape, -2, dtype=torch.int16, device="cuda")
    out_float = torch.full(shape, -1.0, dtype=torch.float32, device="cuda")
    nI, nO, nT = rI[0].numel(), rO[0].numel(), out_fused[0].numel()
    # bytes moved, from the code: the fused pair reads I and O once, writes and reads S, writes the target; the chain writes and
    # reads OI, S, ST and OT as well (five inner-sized and five target-sized passes, the outer read twice)
    moved = {"typed_fused": 2 * nz * (3 * nI + nO + nT), "float_fused": 4 * nz * (3 * nI + nO + nT), "typed_chain": 2 * nz * (5 * nI + 2 * nO + 5 * nT)}
    src = torch.zeros(moved["typed_fused"] // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    path = [None]

    def typed_fused():
        path[0] = plan.apply_typed_device(rI.data_ptr(), pI, rO.data_ptr(), pO, nz, out_fused.data_ptr(), st)

    forms = (("typed_fused", typed_fused),
             ("typed_chain", lambda: plan.apply_typed_chain_device(rI.data_ptr(), pI, rO.data_ptr(), pO, nz, out_chain.data_ptr(), st)),
             ("float_fused", lambda: plan.apply_device(fI.data_ptr(), fO.data_ptr(), nz, out_float.data_ptr(), st)),
             ("copy", lambda: dst.copy_(src)))
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_fused, out_chain))
    assert same, "the typed entry's result differs from the chain's"
    unpacked = torch.where(out_fused == int(pI.fill), torch.full_like(out_float, NAN), out_fused.double().mul(pI.scale).add(pI.offset).float())
    both = ~(unpacked.isnan() | out_float.isnan())
    float_diff = float((unpacked - out_float)[both].abs().max())
    nan_same = bool(torch.equal(unpacked.isnan(), out_float.isnan()))
    del unpacked, both
    t = {k: [] for k, _ in forms}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for rep in range(a.warmup + a.reps):
        for form, fn in forms:
            e0, e1 = ev(), ev()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                t[form].append(e0.elapsed_time(e1))
    ms = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: float(max(v) - min(v)) for k, v in t.items()}
    moved["copy"] = 2 * src.numel()
    beyond = lambda slow, fast: bool(ms[slow] - ms[fast] > spread[slow] + spread[fast])
    r = {"case": "merge on packed shorts, bilinear, LINEAR(5, 2), 1 % fill values in the inner", "slices": nz, "inner": list(INNER), "outer": list(OUTER),
         "target": [int(tx.size), int(ty.size)], "path": path[0], "typed_fused_equals_typed_chain_byte_for_byte": same,
         "float_fused_against_typed_fused": {"undefined_cells_agree": nan_same, "max_abs_difference_of_values": float_diff,
                                             "note": "the float entry blends raw values as floats and rounds once; half a count of the inner's packing is 0.005"},
         "defined_share_of_output": float((out_fused != int(pI.fill)).float().mean()),
         "ms_median": ms, "ms_spread_max_minus_min": spread, "ms_min": {k: float(min(v)) for k, v in t.items()},
         "ms_every_call": {k: [round(float(x), 4) for x in v] for k, v in t.items()},
         "bytes_moved": moved, "bytes_formula": {"typed_fused": "2*nz*(3*I + O + T): I read, S written and read, O read, T written",
                                                 "float_fused": "4*nz*(3*I + O + T)", "typed_chain": "2*nz*(5*I + 2*O + 5*T)",
                                                 "copy": "typed_fused's bytes, half read and half written"},
         "TB_per_s": {k: moved[k] / ms[k] / 1e9 for k in ms},
         "typed_chain_over_typed_fused": ms["typed_chain"] / ms["typed_fused"], "float_fused_over_typed_fused": ms["float_fused"] / ms["typed_fused"],
         "typed_fused_over_copy": ms["typed_fused"] / ms["copy"],
         "faster_beyond_spread": {"typed_fused_than_typed_chain": beyond("typed_chain", "typed_fused"),
                                  "typed_fused_than_float_fused": beyond("float_fused", "typed_fused")},
         "device": torch.cuda.get_device_name(0)}
    # ---- the two elementwise typed kernels on one short / float pair each (the inner's shorts against a float field on the inner
    # grid, the result in shorts: 2 + 4 + 2 bytes per cell), against a device copy of the same bytes, alternating
    del src, dst, out_fused, out_chain, out_float
    pF = fa.Packing(fa.CDM_FLOAT, NAN, 1.0, 0.0)
    n = rI.numel()
    out_e = torch.empty_like(rI)
    src = torch.zeros(4 * n, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    eforms = (("border_smooth_typed", lambda: fa.border_smooth_typed_device(rI.data_ptr(), pI, fI.data_ptr(), pF, out_e.data_ptr(), INNER[0], INNER[1], nz, 5, 2, True, st)),
              ("overlay_typed", lambda: fa.overlay_typed_device(rI.data_ptr(), pI, fI.data_ptr(), pF, out_e.data_ptr(), n, st)),
              ("copy", lambda: dst.copy_(src)))
    te = {k: [] for k, _ in eforms}
    for rep in range(a.warmup + a.reps):
        for form, fn in eforms:
            e0, e1 = ev(), ev()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                te[form].append(e0.elapsed_time(e1))
    mse = {k: float(np.median(v)) for k, v in te.items()}
    r["elementwise_short_float"] = {"cells": n, "bytes_moved": 8 * n, "bytes_formula": "(2 + 4 + 2) * nz * I; the copy moves the same bytes, half read and half written",
                                    "ms_median": mse, "ms_min": {k: float(min(v)) for k, v in te.items()},
                                    "ms_spread_max_minus_min": {k: float(max(v) - min(v)) for k, v in te.items()},
                                    "TB_per_s": {k: 8 * n / mse[k] / 1e9 for k in mse}, "over_copy": {k: mse[k] / mse["copy"] for k in mse if k != "copy"}}
    print(json.dumps(r), flush=True)
    what = ("One MI355X, device resident; the forms alternate launch by launch in one process on the same buffers; per form the median of %d "
            "timed calls after %d of warm-up, HIP events around one call (the stream-ordered allocation of the temporaries included).  "
            "faster_beyond_spread: the medians differ by more than the two spreads (max - min) together." % (a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"script": "scripts/bench_merge_typed.py", "what": what, "reps": a.reps, "warmup": a.warmup, "results": [r]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
