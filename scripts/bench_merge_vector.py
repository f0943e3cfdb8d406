#!/usr/bin/env python3
"""Grid merging of an x/y vector pair (fimex_amd_merge_apply_vector_device) on the workload of scripts/bench_merge.py: 65 pairs, a
2000 x 2000 inner grid centred in a 1000 x 750 outer grid of four times the step, the target the inner grid continued over the
outer one (3996 x 2996), bilinear on all three plans, LINEAR(5, 2), 1 % NaN in each inner component, a smooth angle field per grid.

Four forms alternate launch by launch in one process on the same buffers:
  fused        fimex_amd_merge_apply_vector_device, the two fused pair kernels
  chain        fimex_amd_merge_apply_vector_chain_device: the pair regridded and rotated three times, border_smooth twice, overlay
               twice, on stream-ordered temporaries -- the kernels that served a pair before the fused entry
  two_scalar   fimex_amd_merge_apply_device once per component: what the pair costs without its rotations (another result)
  copy         a device copy of the algorithmic bytes (half read, half written): both pairs read once, the output pair written
               once, the three (m0, m1) arrays read once
Before timing, the fused result is compared with the chain's bit for bit on the device.  Per form: median, min and max of --reps
timed calls after --warmup, HIP events around one call (the stream-ordered allocation of the temporaries included), and every
call's time, so that a stalled allocation shows.  Writes profiles/merge_vector_65.json (or --out) and prints one JSON line.

usage: python scripts/bench_merge_vector.py [--reps 20] [--warmup 3] [--nz 65] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_vector_65.json"))
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

    Iu, Iv = field(INNER[0], INNER[1], i0[0], i0[1], 1.0, 0.0), field(INNER[0], INNER[1], i0[0], i0[1], 1.0, 1.3)
    for f in (Iu, Iv):
        f[torch.rand(f.shape, device="cuda", generator=gen) < 0.01] = NAN
    Ou, Ov = field(OUTER[0], OUTER[1], 0., 0., STEP_O, 0.0), field(OUTER[0], OUTER[1], 0., 0., STEP_O, 1.3)
    shape = (nz, ty.size, tx.size)
    out = {k: [torch.full(shape, fill - c, dtype=torch.float32, device="cuda") for c in (0, 1)] for k, fill in (("fused", -1.), ("chain", -3.), ("two_scalar", -5.))}
    nI, nO, nT = Iu[0].numel(), Ou[0].numel(), out["fused"][0][0].numel()
    alg = 4 * nz * 2 * (nI + nO + nT) + 16 * (nI + 2 * nT)
    src = torch.zeros(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    ins = [t.data_ptr() for t in (Iu, Iv, Ou, Ov)]

    def two_scalar():
        plan.apply_device(ins[0], ins[2], nz, out["two_scalar"][0].data_ptr(), st)
        plan.apply_device(ins[1], ins[3], nz, out["two_scalar"][1].data_ptr(), st)

    forms = (("fused", lambda: plan.apply_vector_device(*rot, *ins, nz, out["fused"][0].data_ptr(), out["fused"][1].data_ptr(), st)),
             ("chain", lambda: plan.apply_vector_chain_device(*rot, *ins, nz, out["chain"][0].data_ptr(), out["chain"][1].data_ptr(), st)),
             ("two_scalar", two_scalar),
             ("copy", lambda: dst.copy_(src)))
    for _, fn in forms:
        fn()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(f.view(torch.int32), c.view(torch.int32))) for f, c in zip(out["fused"], out["chain"]))
    assert same, "the fused entry's result differs from the chain's"
    finite = float(torch.isfinite(out["fused"][0]).float().mean())
    lo, hi = float(torch.nan_to_num(out["fused"][0], nan=0.).min()), float(torch.nan_to_num(out["fused"][0], nan=0.).max())
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
    # bytes moved, from the code: the fused pair reads I and O once, writes and reads S, writes the target, all twice, and reads the
    # three matrices; the chain writes and reads OI, S, ST and OT as well
    moved = {"fused": 4 * nz * 2 * (3 * nI + nO + nT) + 16 * (nI + 2 * nT), "copy": 2 * src.numel()}
    r = {"case": "merge of a vector pair, bilinear, LINEAR(5, 2), 1 % NaN in each inner component, three smooth angle fields", "pairs": nz,
         "inner": list(INNER), "outer": list(OUTER), "target": [int(tx.size), int(ty.size)], "reps": a.reps, "warmup": a.warmup,
         "fused_equals_chain_bit_for_bit": same, "finite_share_of_output_u": finite, "output_u_min": lo, "output_u_max": hi,
         "ms_median": ms, "ms_min": {k: float(min(v)) for k, v in t.items()}, "ms_max": {k: float(max(v)) for k, v in t.items()},
         "ms_every_call": {k: [round(float(x), 4) for x in v] for k, v in t.items()},
         "algorithmic_bytes": alg, "algorithmic_bytes_formula": "4*nz*2*(ix*iy + ox*oy + tx*ty) [both pairs read, the output pair written] + 16*(ix*iy + 2*tx*ty) [(m0, m1) of R_oi, R_st, R_ot]",
         "scratch_bytes": 4 * nz * 2 * nI, "scratch": "the smoothed pair, written once by merge_smooth_vector and read by merge_overlay_vector; not part of the algorithmic bytes",
         "bytes_moved": moved, "TB_per_s_on_algorithmic_bytes": {k: alg / ms[k] / 1e9 for k in ms},
         "chain_over_fused": ms["chain"] / ms["fused"], "fused_over_two_scalar": ms["fused"] / ms["two_scalar"], "fused_over_copy": ms["fused"] / ms["copy"],
         "fused_median_not_above_chain_median": bool(ms["fused"] <= ms["chain"]),
         "every_fused_call_below_every_chain_call": bool(max(t["fused"]) < min(t["chain"])),
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r), flush=True)
    what = ("One MI355X, device resident; the forms alternate launch by launch in one process on the same buffers; per form the median, min and max "
            "of %d timed calls after %d of warm-up, HIP events around one call (the stream-ordered allocation of the temporaries included)." % (a.reps, a.warmup))
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.update({"script": "scripts/bench_merge_vector.py", "what": what, "results": [r]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
