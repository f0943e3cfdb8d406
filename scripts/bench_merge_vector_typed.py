#!/usr/bin/env python3
"""Grid merging of a packed x/y vector pair (fimex_amd_merge_apply_vector_typed_device) on the workload of scripts/bench_merge.py:
65 pairs, a 2000 x 2000 inner grid centred in a 1000 x 750 outer grid of four times the step, the target the inner grid continued
over the outer one (3996 x 2996), bilinear on all three plans, LINEAR(5, 2), 1 % fill values in each inner component, a smooth
angle field per grid.  All four fields are shorts, each with its own packing (inner u, inner v, outer u, outer v):
  S -32768 0.01 0 | S -32767 0.01 0 | S -32767 0.02 0 | S -32768 0.05 -3

Four forms alternate launch by launch in one process on the same buffers:
  fused        fimex_amd_merge_apply_vector_typed_device, the two fused pair kernels on shorts (path 1)
  chain        fimex_amd_merge_apply_vector_typed_chain_device: the pair regridded and rotated three times on its stored type, the
               typed smoothing twice, the typed overlay twice, on stream-ordered temporaries of the stored types -- the launches
               that served a packed pair before the fused entry, as one call
  two_scalar   fimex_amd_merge_apply_typed_device once per component: what the pair costs without its rotations (another result)
  copy         a device copy of the fused form's bytes (half read, half written)
Before timing, the fused result is compared with the chain's byte for byte on the device.  Per form: median, min and max of --reps
timed calls after --warmup, HIP events around one call (the stream-ordered allocations included), every call's time, and the calls
above 0.4 s, so that a stalled allocation shows.  Writes profiles/merge_vector_typed.json (or --out) and prints one JSON line.

usage: python scripts/bench_merge_vector_typed.py [--reps 20] [--warmup 3] [--nz 65] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INNER = (2000, 2000)   # nx, ny, step 1
OUTER = (1000, 750)    # nx, ny, step 4
STEP_O = 4.0
NAN = float("nan")
STALL_MS = 400.0


def index_positions(src0, src_step, dst_x, dst_y):
    """fractional (column, row) of the mesh of two target axes on a source grid with origin src0 and one step"""
    X, Y = np.meshgrid(dst_x, dst_y)
    return ((X - src0[0]) / src_step).ravel(), ((Y - src0[1]) / src_step).ravel()


def rotation(x, y, phase):
    """the reference's double[4 * cells] of an angle field that varies smoothly over the grid (about a radian across it)"""
    X, Y = np.meshgrid(x, y)
    phi = 0.6 * np.sin(X / 1500. + phase) + 0.4 * np.cos(Y / 1100. - phase)
    m = np.empty(phi.shape + (4,), np.float64)
    m[..., 0], m[..., 1], m[..., 2], m[..., 3] = np.cos(phi), np.sin(phi), -np.sin(phi), phi
    return m.ravel()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nz", type=int, default=65)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_vector_typed.json"))
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
    rot = (fa.VectorPlan(rotation(ix, iy, 0.0), INNER[0], INNER[1]), fa.VectorPlan(rotation(tx, ty, 0.7), tx.size, ty.size),
           fa.VectorPlan(rotation(tx, ty, 1.9), tx.size, ty.size))
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)

    def field(nx, ny, x0, y0, step, phase):
        jj = (y0 + step * torch.arange(ny, dtype=torch.float32, device="cuda"))[None, :, None]
        ii = (x0 + step * torch.arange(nx, dtype=torch.float32, device="cuda"))[None, None, :]
        zz = torch.arange(nz, dtype=torch.float32, device="cuda")[:, None, None]
        return (8. * torch.sin(0.004 * ii + 0.1 * zz + phase) * torch.cos(0.005 * jj - phase) + 0.3 * torch.randn((nz, ny, nx), device="cuda", generator=gen)).contiguous()

    packings = (fa.Packing(fa.CDM_SHORT, -32768.0, 0.01, 0.0), fa.Packing(fa.CDM_SHORT, -32767.0, 0.01, 0.0),
                fa.Packing(fa.CDM_SHORT, -32767.0, 0.02, 0.0), fa.Packing(fa.CDM_SHORT, -32768.0, 0.05, -3.0))

    def packed(f, p):  # the field as a writer packs it, NaN as the fill value
        raw = torch.empty(f.shape, dtype=torch.int16, device="cuda")
        fa.convert_scaled_device(f.data_ptr(), fa.CDM_FLOAT, f.numel(), NAN, 1.0, 0.0, fa.CDM_SHORT, p.fill, p.scale, p.offset, raw.data_ptr(), st)
        torch.cuda.synchronize()
        return raw

    floats = [field(INNER[0], INNER[1], i0[0], i0[1], 1.0, 0.0), field(INNER[0], INNER[1], i0[0], i0[1], 1.0, 1.3),
              field(OUTER[0], OUTER[1], 0., 0., STEP_O, 0.0), field(OUTER[0], OUTER[1], 0., 0., STEP_O, 1.3)]
    for f in floats[:2]:
        f[torch.rand(f.shape, device="cuda", generator=gen) < 0.01] = NAN
    raws = [packed(f, p) for f, p in zip(floats, packings)]
    del floats
    shape = (nz, ty.size, tx.size)
    out = {k: [torch.full(shape, fill - c, dtype=torch.int16, device="cuda") for c in (0, 1)] for k, fill in (("fused", -1), ("chain", -3), ("two_scalar", -5))}
    nI, nO, nT = raws[0][0].numel(), raws[2][0].numel(), out["fused"][0][0].numel()
    # bytes moved, from the code.  fused: I read, S written and read, O read, T written, per component, and the three (m0, m1)
    # arrays; chain: per component OI, S, ST and OT written and read as well, the outer read twice
    moved = {"fused": 2 * nz * 2 * (3 * nI + nO + nT) + 16 * (nI + 2 * nT), "chain": 2 * nz * 2 * (5 * nI + 2 * nO + 5 * nT) + 16 * (nI + 2 * nT)}
    src = torch.zeros(moved["fused"] // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    moved["copy"] = 2 * src.numel()
    fields = [x for r, p in zip(raws, packings) for x in (r.data_ptr(), p)]
    path = [None]

    def fused():
        path[0] = plan.apply_vector_typed_device(*rot, *fields, nz, out["fused"][0].data_ptr(), out["fused"][1].data_ptr(), st)

    def two_scalar():
        plan.apply_typed_device(raws[0].data_ptr(), packings[0], raws[2].data_ptr(), packings[2], nz, out["two_scalar"][0].data_ptr(), st)
        plan.apply_typed_device(raws[1].data_ptr(), packings[1], raws[3].data_ptr(), packings[3], nz, out["two_scalar"][1].data_ptr(), st)

    forms = (("fused", fused),
             ("chain", lambda: plan.apply_vector_typed_chain_device(*rot, *fields, nz, out["chain"][0].data_ptr(), out["chain"][1].data_ptr(), st)),
             ("two_scalar", two_scalar),
             ("copy", lambda: dst.copy_(src)))
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(f, c)) for f, c in zip(out["fused"], out["chain"]))
    assert same, "the fused entry's result differs from the chain's"
    defined = [float((o != int(p.fill)).float().mean()) for o, p in zip(out["fused"], packings)]
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
    r = {"case": "merge of a packed vector pair (shorts, four packings), bilinear, LINEAR(5, 2), 1 % fill values in each inner component, three smooth angle fields",
         "pairs": nz, "inner": list(INNER), "outer": list(OUTER), "target": [int(tx.size), int(ty.size)], "reps": a.reps, "warmup": a.warmup,
         "path": path[0], "fused_equals_chain_byte_for_byte": same, "defined_share_of_output": defined,
         "ms_median": ms, "ms_min": {k: float(min(v)) for k, v in t.items()}, "ms_max": {k: float(max(v)) for k, v in t.items()},
         "calls_above_0.4_s": {k: int(sum(x > STALL_MS for x in v)) for k, v in t.items()},
         "ms_every_call": {k: [round(float(x), 4) for x in v] for k, v in t.items()},
         "bytes_moved": moved,
         "bytes_formula": {"fused": "2*nz*2*(3*I + O + T) + 16*(I + 2*T): per component I read, S written and read, O read, T written; (m0, m1) of R_oi, R_st, R_ot",
                           "chain": "2*nz*2*(5*I + 2*O + 5*T) + 16*(I + 2*T)", "copy": "fused's bytes, half read and half written"},
         "TB_per_s": {k: moved[k] / ms[k] / 1e9 for k in moved},
         "chain_over_fused": ms["chain"] / ms["fused"], "fused_over_two_scalar": ms["fused"] / ms["two_scalar"], "fused_over_copy": ms["fused"] / ms["copy"],
         "fused_median_not_above_chain_median": bool(ms["fused"] <= ms["chain"]),
         "every_fused_call_below_every_chain_call": bool(max(t["fused"]) < min(t["chain"])),
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r), flush=True)
    what = ("One MI355X, device resident; the forms alternate launch by launch in one process on the same buffers; per form the median, min and max "
            "of %d timed calls after %d of warm-up, HIP events around one call (the stream-ordered allocation of the temporaries included)." % (a.reps, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"script": "scripts/bench_merge_vector_typed.py", "what": what, "results": [r]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
