#!/usr/bin/env python3
"""Vertical interpolation of 65 model levels to 20 pressure levels on 2000 x 2000 (method log), device-resident and HIP-event
timed: input levels as HYBRID_SIGMA_AP (computed in the kernel from ps) and as an explicit FIELD, nt = 1 and 4.
Per case: median of --launches calls after a warm-up, the algorithmic bytes (data in + out + ps, or + the level field) and the
rate they give, and -- the yardstick -- the time of a device-to-device copy that moves the same number of bytes (half of them
read, half written) taken in the same run.  Writes profiles/vertical_65to20.json (or --out) and prints one JSON line per case.
--groups 4,8 also times the kernel with 8 output levels per walk of a column instead of 4 (tuning build).
usage: python scripts/bench_vertical.py [--nt 1,4] [--kinds ap,field] [--launches 20] [--groups 4] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_others import timed

NX = NY = 2000
NZI, NZO = 65, 20
LEVEL1 = np.array([10., 20., 30., 50., 70., 100., 150., 200., 250., 300., 400., 500., 600., 700., 800., 850., 900., 925., 950., 1000.])


def hybrid_coefficients():
    """65 levels from 10 hPa to the surface: ap + b * ps with b growing towards the ground."""
    v = 10.0 * 100.0 ** (np.arange(NZI) / (NZI - 1.0))
    b = 0.9 * (v / 1000.0) ** 2
    return v - b * 1000.0, b


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--nt", default="1,4")
    ap_.add_argument("--kinds", default="ap,field")
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--groups", default="4")
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical_65to20.json"))
    args = ap_.parse_args()
    import torch
    from fimex_amd import capi as fa
    groups = [int(g) for g in args.groups.split(",")]
    if groups != [4]:
        fa.use_tuning_build(True)  # the only build that reads FIMEX_AMD_VERTICAL_GROUP
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    plane = NX * NY
    ap, b = hybrid_coefficients()
    results = []
    for nt in [int(t) for t in args.nt.split(",")]:
        gen = torch.Generator(device="cuda"); gen.manual_seed(nt)
        jj = torch.arange(NY, device="cuda", dtype=torch.float32)[:, None]
        ii = torch.arange(NX, device="cuda", dtype=torch.float32)[None, :]
        terrain = 0.5 + 0.5 * torch.sin(0.011 * ii) * torch.cos(0.007 * jj)  # surface pressure from 600 (mountains) to 1040 hPa
        ps = torch.stack([600. + 440. * terrain + 3. * torch.randn((NY, NX), device="cuda", generator=gen) + 5. * t for t in range(nt)]).contiguous()
        data = 280. + torch.randn((nt, NZI, NY, NX), device="cuda", generator=gen)
        data[torch.rand((nt, NZI, NY, NX), device="cuda", generator=gen) < 0.05] = float("nan")
        out = torch.empty((nt, NZO, NY, NX), dtype=torch.float32, device="cuda")
        hybrid = fa.VerticalLevels.hybrid_sigma_ap(ap, b, ps.data_ptr())
        for kind in args.kinds.split(","):
            if kind == "field":
                field = torch.empty((nt, NZI, NY, NX), dtype=torch.float32, device="cuda")
                fa.vertical_levels_device(hybrid, NX, NY, nt, field.data_ptr(), st)
                levels = fa.VerticalLevels.from_field(field.data_ptr(), NZI)
                alg = 4 * nt * plane * (NZI + NZO + NZI)
            else:
                field = None
                levels = hybrid
                alg = 4 * nt * plane * (NZI + NZO + 1)
            src = torch.empty(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
            src.zero_()
            copy_ms, copy_min = timed(torch, lambda: dst.copy_(src), reps=args.launches, warm=3)
            del src, dst
            for g in groups:
                os.environ["FIMEX_AMD_VERTICAL_GROUP"] = str(g)
                call = lambda: fa.vertical_interpolate_device(fa.VINT_METHOD_LOG, NX, NY, nt, data.data_ptr(), levels, out.data_ptr(),
                                                              level1=LEVEL1, stream=st)
                ms, mn = timed(torch, call, reps=args.launches, warm=3)
                torch.cuda.synchronize()
                r = {"case": "%d -> %d levels, %d x %d, nt = %d, method log, input levels %s" % (
                         NZI, NZO, NX, NY, nt, "HYBRID_SIGMA_AP" if kind == "ap" else "FIELD"),
                     "levels_per_walk": g, "launches": args.launches, "ms_median": ms, "ms_min": mn,
                     "algorithmic_bytes": alg, "TBps": alg / ms / 1e9,
                     "copy_payload_bytes": alg // 2, "copy_ms_median": copy_ms, "copy_ms_min": copy_min, "copy_TBps": alg / copy_ms / 1e9,
                     "kernel_over_copy": ms / copy_ms,
                     "defined_share_of_output": float((~torch.isnan(out)).float().mean()), "device": torch.cuda.get_device_name(0)}
                print(json.dumps(r), flush=True)
                results.append(r)
            del field
        del data, out, ps
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"script": "scripts/bench_vertical.py", "timing": "HIP events around one call, median of the launches after 3 warm-up calls",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
