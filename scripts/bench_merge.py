#!/usr/bin/env python3
"""Grid merging (fimex_amd_merge_apply_device) on 65 slices, device-resident and HIP-event timed: median of --launches calls after
3 warm-up calls.  A 2000 x 2000 inner grid centred in a 1000 x 750 outer grid of four times the step, the target the inner grid
continued over the outer one (extendInnerAxis, about 4000 x 3000), bilinear, LINEAR(5, 2) smoothing, 1 % NaN in the inner field.
The algorithmic bytes are the inner and the outer read once and the target written once; the smoothed inner field that passes
between the two fused kernels is counted separately.  Two yardsticks are taken in the same run: a device-to-device copy that moves
the algorithmic bytes (half read, half written), and fimex_amd_merge_apply_chain_device (the three plain applies and the two
elementwise kernels on temporaries) on the same buffers; the two results are compared bit for bit.  Writes the "results" of
profiles/merge_65.json (or --out), keeping the file's other keys, and prints one JSON line.

usage: python scripts/bench_merge.py [--launches 20] [--nz 65] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

INNER = (2000, 2000)   # nx, ny, step 1
OUTER = (1000, 750)    # nx, ny, step 4
STEP_O = 4.0


def update(path, key, value):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["script"] = "scripts/bench_merge.py"
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def index_positions(src0, src_step, dst_x, dst_y):
    """fractional (column, row) of the mesh of two target axes on a source grid with origin src0 and one step"""
    X, Y = np.meshgrid(dst_x, dst_y)
    return ((X - src0[0]) / src_step).ravel(), ((Y - src0[1]) / src_step).ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--nz", type=int, default=65)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_65.json"))
    args = ap.parse_args()
    import torch
    import merge_ref as mr
    from bench_others import timed
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    nz = args.nz
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

    I = field(INNER[0], INNER[1], i0[0], i0[1], 1.0)
    I[torch.rand(I.shape, device="cuda", generator=gen) < 0.01] = float("nan")
    O = field(OUTER[0], OUTER[1], 0., 0., STEP_O)
    fused = torch.full((nz, ty.size, tx.size), -1.0, dtype=torch.float32, device="cuda")
    chain = torch.full((nz, ty.size, tx.size), -2.0, dtype=torch.float32, device="cuda")
    alg = 4 * nz * (I[0].numel() + O[0].numel() + fused[0].numel())
    src = torch.empty(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.zero_()
    copy_ms, copy_min = timed(torch, lambda: dst.copy_(src), reps=args.launches, warm=3)
    del src, dst
    ms, mn = timed(torch, lambda: plan.apply_device(I.data_ptr(), O.data_ptr(), nz, fused.data_ptr(), st), reps=args.launches, warm=3)
    chain_ms, chain_min = timed(torch, lambda: plan.apply_chain_device(I.data_ptr(), O.data_ptr(), nz, chain.data_ptr(), st), reps=args.launches, warm=3)
    torch.cuda.synchronize()
    same = bool(torch.equal(fused.view(torch.int32), chain.view(torch.int32)))
    r = {"case": "merge, bilinear, LINEAR(5, 2), 1 % NaN in the inner", "slices": nz, "inner": list(INNER), "outer": list(OUTER),
         "target": [int(tx.size), int(ty.size)], "launches": args.launches, "ms_median": ms, "ms_min": mn,
         "algorithmic_bytes": alg, "algorithmic_bytes_formula": "4*nz*(ix*iy [inner] + ox*oy [outer] + tx*ty [target])", "TBps": alg / ms / 1e9,
         "scratch_bytes": 4 * nz * I[0].numel(), "scratch": "the smoothed inner field, written once by merge_smooth and read by merge_overlay; "
                                                            "not part of the algorithmic bytes",
         "copy_payload_bytes": alg // 2, "copy_ms_median": copy_ms, "copy_ms_min": copy_min, "copy_TBps": alg / copy_ms / 1e9,
         "fused_over_copy": ms / copy_ms, "chain_ms_median": chain_ms, "chain_ms_min": chain_min, "chain_over_fused": chain_ms / ms,
         "fused_equals_chain_bit_for_bit": same, "finite_share_of_output": float(torch.isfinite(fused).float().mean()),
         "output_min": float(torch.nan_to_num(fused, nan=300.).min()), "output_max": float(torch.nan_to_num(fused, nan=0.).max()),
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r), flush=True)
    update(args.out, "timing", "HIP events around one call, median of the launches after 3 warm-up calls")
    update(args.out, "results", [r])


if __name__ == "__main__":
    main()
