#!/usr/bin/env python3
"""The vertical level converters on 65 levels, 2000 x 2000, nt = 1, device-resident and HIP-event timed: the hypsometric
integration to height above ground with HYBRID_SIGMA_AP pressure (with and without humidity) and with FIELD pressure, the
standard-atmosphere altitude of HYBRID_SIGMA_AP pressure, and the ocean s-coordinate depth (generation 2, with eta).
Per case: median of --launches calls after 3 warm-up calls, the algorithmic bytes (every plane read once plus the output; the
formula is in the record) and the rate they give, and -- the yardstick -- the time of a device-to-device copy that moves the same
number of bytes (half of them read, half written) taken in the same run.  Writes profiles/vertical_levels_65.json (or --out) and
prints one JSON line per case.
usage: python scripts/bench_vertical_levels.py [--cases hybrid_q,hybrid_dry,field_q,standard,ocean] [--launches 20] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_others import timed

NX = NY = 2000
NZ = 65
G = 9.80665


def hybrid_coefficients():
    """65 levels from about 8 hPa down to just above the surface, index 0 at the top: ap + b * ps below ps for every ps >= 600."""
    eta = (np.arange(NZ) + 0.5) / NZ
    b = eta ** 2
    return 1000.0 * (eta - b) + 0.1, b


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--cases", default="hybrid_q,hybrid_dry,field_q,standard,ocean")
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical_levels_65.json"))
    args = ap_.parse_args()
    import torch
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    plane = NX * NY
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    jj = torch.arange(NY, device="cuda", dtype=torch.float32)[:, None]
    ii = torch.arange(NX, device="cuda", dtype=torch.float32)[None, :]
    terrain = 0.5 + 0.5 * torch.sin(0.011 * ii) * torch.cos(0.007 * jj)  # surface pressure from 600 (mountains) to 1040 hPa
    ps = (600. + 440. * terrain).reshape(1, NY, NX).contiguous()
    sgp = (G * 3000. * (1040. - ps) / 440.).contiguous()
    topo = sgp[0].double().contiguous()
    eta = torch.tensor((np.arange(NZ) + 0.5) / NZ, device="cuda", dtype=torch.float32)[None, :, None, None]
    T = (210. + 80. * eta + 2. * torch.randn((1, NZ, NY, NX), device="cuda", generator=gen)).contiguous()
    q = (0.015 * eta ** 3 * torch.rand((1, NZ, NY, NX), device="cuda", generator=gen)).contiguous()
    out = torch.empty((1, NZ, NY, NX), dtype=torch.float32, device="cuda")
    ap, b = hybrid_coefficients()
    hybrid = fa.VerticalLevels.hybrid_sigma_ap(ap, b, ps.data_ptr())
    vol, pl = 4 * plane * NZ, 4 * plane
    results = []

    def run(name, call, alg, formula, keep=None):
        src = torch.empty(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        src.zero_()
        copy_ms, copy_min = timed(torch, lambda: dst.copy_(src), reps=args.launches, warm=3)
        del src, dst
        out.fill_(-1.0)
        ms, mn = timed(torch, call, reps=args.launches, warm=3)
        torch.cuda.synchronize()
        r = {"case": name, "levels": NZ, "nx": NX, "ny": NY, "nt": 1, "launches": args.launches, "ms_median": ms, "ms_min": mn,
             "algorithmic_bytes": alg, "algorithmic_bytes_formula": formula, "TBps": alg / ms / 1e9,
             "copy_payload_bytes": alg // 2, "copy_ms_median": copy_ms, "copy_ms_min": copy_min, "copy_TBps": alg / copy_ms / 1e9,
             "kernel_over_copy": ms / copy_ms, "finite_share_of_output": float(torch.isfinite(out).float().mean()),
             "output_min": float(out.min()), "output_max": float(out.max()), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(r), flush=True)
        results.append(r)

    def integrate(levels, with_q):
        return lambda: fa.vertical_altitude_integrate_device(levels, NX, NY, 1, T.data_ptr(), ps.data_ptr(), sgp.data_ptr(), out.data_ptr(),
                                                             d_specificHumidity=q.data_ptr() if with_q else None,
                                                             surfaceFirst=fa.VORDER_AUTO, d_topo=topo.data_ptr(), topoFactor=-1.0 / G, stream=st)

    for case in args.cases.split(","):
        if case == "hybrid_q":
            run("integration to height, HYBRID_SIGMA_AP pressure, with humidity", integrate(hybrid, True), 3 * vol + 3 * pl + 2 * pl,
                "4*nx*ny*(nz [T] + nz [q] + nz [out] + 3 [ps, sap, sgp]) + 8*nx*ny [topo]")
        elif case == "hybrid_dry":
            run("integration to height, HYBRID_SIGMA_AP pressure, no humidity", integrate(hybrid, False), 2 * vol + 3 * pl + 2 * pl,
                "4*nx*ny*(nz [T] + nz [out] + 3 [ps, sap, sgp]) + 8*nx*ny [topo]")
        elif case == "field_q":
            field = torch.empty((1, NZ, NY, NX), dtype=torch.float32, device="cuda")
            fa.vertical_levels_device(hybrid, NX, NY, 1, field.data_ptr(), st)
            torch.cuda.synchronize()
            run("integration to height, FIELD pressure, with humidity", integrate(fa.VerticalLevels.from_field(field.data_ptr(), NZ), True),
                4 * vol + 2 * pl + 2 * pl, "4*nx*ny*(nz [p] + nz [T] + nz [q] + nz [out] + 2 [sap, sgp]) + 8*nx*ny [topo]")
            del field
        elif case == "standard":
            run("standard altitude of HYBRID_SIGMA_AP pressure",
                lambda: fa.vertical_standard_altitude_device(hybrid, NX, NY, 1, out.data_ptr(), stream=st), vol + pl,
                "4*nx*ny*(nz [out] + 1 [ps])")
        elif case == "ocean":
            s = -(1.0 - (np.arange(NZ) + 0.5) / NZ)
            C = -np.abs(s) ** 1.7
            depth = (5. + 4000. * terrain).double().contiguous()
            zeta = (0.5 * torch.randn((1, NY, NX), device="cuda", generator=gen)).double().contiguous()
            run("ocean s-coordinate depth, generation 2, with eta",
                lambda: fa.vertical_ocean_depth_device(2, NX, NY, 1, s, C, 20.0, depth.data_ptr(), out.data_ptr(), d_eta=zeta.data_ptr(), stream=st),
                vol + 4 * pl, "4*nx*ny*nz [out] + 8*nx*ny*2 [depth, eta as doubles]")
        else:
            raise SystemExit("unknown case " + case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"script": "scripts/bench_vertical_levels.py", "timing": "HIP events around one call, median of the launches after 3 warm-up calls",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
