#!/usr/bin/env python3
"""A vector pair of packed shorts regridded, rotated and packed again: the five existing device launches (to float twice, the float
pair entry, back to short twice; `chain`) against the entry on the stored type (fimex_amd_regrid_apply_vector_typed_device;
`fused`), in one process and on the same buffers, alternating launch by launch.  The chain's float temporaries are allocated
once, outside the timed region.

Geometries: the headline plan of bench.py (4000 x 3000 -> 2000 x 2000) with 100, 25, 8 and 4 pairs; the plan of BASELINE
configs[4] (scripts/bench_c5_chain.py: 3000 x 3000 polar stereographic -> 3000 x 3000 lat/lon) with 16 pairs.  Nearest and
bilinear.  Per case: the fused result is compared with the chain's byte for byte, then after warm-up the median of REPS timed
repetitions of each form from HIP events; algorithmic bytes of both, TB/s, the ratio chain / fused, and a device copy scaled to
the fused form's bytes.

usage: python scripts/bench_vector_regrid_typed.py [--reps 20] [--warmup 3] [--out profiles/vector_regrid_typed.json]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_regrid_typed.json"))
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed repetitions"
    import torch
    from fimex_amd import capi as fa
    import bench, workloads
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    ev = lambda: torch.cuda.Event(enable_timing=True)
    results = []
    SHORT, U_BAD, V_BAD = fa.CDM_SHORT, -32768.0, 32767.0

    def smooth_matrix(ox, oy):  # (cos, sin, -sin, phi) of a smooth angle field: the kernels' time does not depend on the values
        j, i = np.meshgrid(np.arange(oy), np.arange(ox), indexing="ij")
        phi = (0.9 * np.sin(0.005 * i) + 0.7 * np.cos(0.003 * j)).ravel()
        return np.stack([np.cos(phi), np.sin(phi), -np.sin(phi), phi], axis=1).ravel()

    def pack(d_f, scale, bad):  # float slices -> shorts as a writer packs them (scale_factor), NaN -> the fill value
        out = torch.empty(d_f.shape, dtype=torch.int16, device="cuda")
        for k in range(d_f.shape[0]):
            out[k] = torch.where(d_f[k].isnan(), torch.full_like(d_f[k], bad), (d_f[k] * scale).round().clamp(-32000, 32000)).to(torch.int16)
        return out

    def run(name, geometry, method, plan, vec, d_u, d_v, nz, tmp):
        inL, outL = plan.inX * plan.inY, plan.outX * plan.outY
        bufs = [torch.empty((nz, plan.outY, plan.outX), dtype=torch.int16, device="cuda") for _ in range(4)]
        cu, cv, fu, fv = bufs
        ptr = [b.data_ptr() for b in bufs]
        t_u, t_v, t_uo, t_vo = (x.data_ptr() for x in tmp)  # the chain's float temporaries, sized for the longest batch

        def chain():
            fa.data2interpolation_device(d_u.data_ptr(), SHORT, nz * inL, U_BAD, t_u, st)
            fa.data2interpolation_device(d_v.data_ptr(), SHORT, nz * inL, V_BAD, t_v, st)
            plan.apply_vector_device(vec, t_u, t_v, nz, t_uo, t_vo, st)
            fa.interpolation2data_device(t_uo, nz * outL, SHORT, U_BAD, ptr[0], st)
            fa.interpolation2data_device(t_vo, nz * outL, SHORT, V_BAD, ptr[1], st)

        def fused():
            return plan.apply_vector_typed_device(vec, d_u.data_ptr(), SHORT, U_BAD, d_v.data_ptr(), SHORT, V_BAD, nz, ptr[2], ptr[3], st)

        chain(); path = fused(); torch.cuda.synchronize()
        ok = bool(torch.equal(cu, fu) and torch.equal(cv, fv))
        assert ok, "%s: the fused result differs from the chain's" % name
        defined = float(((fu != int(U_BAD)) & (fv != int(V_BAD))).float().mean().item())
        t = {"chain": [], "fused": [], "copy": []}
        info = plan.info()
        plan_bytes, matrix_bytes = info["planBytes"], 16 * outL
        bytes_fused = 2 * nz * 2 * (inL + outL) + plan_bytes + matrix_bytes
        # to float: 2 + 4 per source cell and component; the float pair entry: 4 + 4; back: 4 + 2 per output cell and component
        bytes_chain = 2 * nz * ((2 + 4 + 4) * inL + (4 + 4 + 2) * outL) + plan_bytes + matrix_bytes
        src = d_u.view(-1)[: bytes_fused // 4]  # bytes_fused / 2 bytes of shorts
        dst = torch.empty_like(src)
        for rep in range(a.warmup + a.reps):
            for form, fn in (("chain", chain), ("fused", fused), ("copy", lambda: dst.copy_(src))):
                e0, e1 = ev(), ev()
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    t[form].append(e0.elapsed_time(e1))
        ms = {k: float(np.median(v)) for k, v in t.items()}
        copy_bytes = 2 * src.numel() * 2
        ms["copy_scaled_to_fused_bytes"] = ms["copy"] * bytes_fused / copy_bytes
        mm = {k: [float(min(v)), float(max(v))] for k, v in t.items()}
        rec = {"case": name, "geometry": geometry, "method": method, "pairs": nz, "path": path, "same_bytes_as_chain": ok,
               "cells_defined_in_both": defined, "ms": ms, "ms_min_max": mm,
               "bytes": {"chain": bytes_chain, "fused": bytes_fused, "plan": plan_bytes, "matrix": matrix_bytes, "copy": copy_bytes},
               "TB_per_s": {"chain": bytes_chain / ms["chain"] / 1e9, "fused": bytes_fused / ms["fused"] / 1e9, "copy": copy_bytes / ms["copy"] / 1e9},
               "chain_over_fused": ms["chain"] / ms["fused"],
               # faster by more than the two spreads together
               "faster_beyond_spread": bool(ms["chain"] - ms["fused"] > (mm["chain"][1] - mm["chain"][0]) + (mm["fused"][1] - mm["fused"][0])),
               "plan": {k: info[k] for k in ("stagedCells", "tileW", "tileH", "undefinedCells")}}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del bufs, cu, cv, fu, fv, src, dst

    # ---- the headline geometry
    wl = workloads.BilinearRotatedPole()
    d_f = bench.make_slices(torch, wl.base_field(), 100)
    d_u = pack(d_f, 100.0, U_BAD)
    d_f -= 280
    d_v = pack(d_f, 100.0, V_BAD)
    del d_f
    tmp = [torch.empty(100 * wl.inX * wl.inY, dtype=torch.float32, device="cuda") for _ in range(2)] + [
        torch.empty(100 * wl.outX * wl.outY, dtype=torch.float32, device="cuda") for _ in range(2)]
    vec = fa.VectorPlan(smooth_matrix(wl.outX, wl.outY), wl.outX, wl.outY)
    headline = "%dx%d -> %dx%d (bench.py headline)" % (wl.inX, wl.inY, wl.outX, wl.outY)
    for method, mname in ((fa.NEAREST_NEIGHBOR, "nearest"), (fa.BILINEAR, "bilinear")):
        plan, _, _ = bench.build_plan(fa, torch, wl, method, st)
        for nz in (100, 25, 8, 4):
            run("headline_%s_%dpairs" % (mname, nz), headline, mname, plan, vec, d_u, d_v, nz, tmp)
        plan.close()
    del d_u, d_v, tmp
    vec.close()
    # ---- BASELINE configs[4], as scripts/bench_c5_chain.py builds it
    n, ox, oy, nz = 3000, 3000, 3000, 16
    stere, geo = "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +R=6371000", "+proj=latlong +R=6371000"
    sx = (np.arange(n) - n / 2 + 0.5) * 1000.0
    sy = (np.arange(n) - n / 2 + 0.5) * 1000.0 - 2.6e6
    lon, lat = np.linspace(-25, 25, ox), np.linspace(52, 78, oy)
    d_px = torch.empty(ox * oy, dtype=torch.float64, device="cuda"); d_py = torch.empty_like(d_px)
    vec = fa.VectorPlan(fa.get_vector_reproject_matrix_host(stere, geo, lon, lat, fa.LONGITUDE, fa.LATITUDE), ox, oy)
    yy, xx = torch.meshgrid(torch.from_numpy(sy).cuda(), torch.from_numpy(sx).cuda(), indexing="ij")
    ang = (1e-6 * xx + 2e-6 * yy).float()
    u0, v0 = 10 * torch.cos(ang), 10 * torch.sin(ang)
    u0[500:900, 1000:1500] = float("nan"); v0[500:900, 1000:1500] = float("nan")
    d_u = pack(torch.stack([u0 * (1 + 0.01 * k) for k in range(nz)]), 1000.0, U_BAD)
    d_v = pack(torch.stack([v0 * (1 + 0.01 * k) for k in range(nz)]), 1000.0, V_BAD)
    del xx, yy, ang, u0, v0
    tmp = [torch.empty(nz * n * n, dtype=torch.float32, device="cuda") for _ in range(2)] + [
        torch.empty(nz * ox * oy, dtype=torch.float32, device="cuda") for _ in range(2)]
    for method, mname in ((fa.NEAREST_NEIGHBOR, "nearest"), (fa.BILINEAR, "bilinear")):
        fa.project_axes_device(geo, stere, np.radians(lon), np.radians(lat), d_px.data_ptr(), d_py.data_ptr(), st)
        fa.points2position_device(d_px.data_ptr(), d_px.numel(), sx, fa.PROJ_AXIS, st)
        fa.points2position_device(d_py.data_ptr(), d_py.numel(), sy, fa.PROJ_AXIS, st)
        plan = fa.RegridPlan.from_device(method, d_px.data_ptr(), d_py.data_ptr(), d_px.numel(), n, n, ox, oy, st)
        run("c5_%s_16pairs" % mname, "3000x3000 polar stereographic -> 3000x3000 lat/lon (BASELINE configs[4])", mname, plan, vec, d_u, d_v, nz, tmp)
        plan.close()
    what = ("A vector pair of shorts regridded, rotated and packed again on one MI355X, device resident: the five existing launches "
            "(fimex_amd_data2interpolation_device twice, fimex_amd_regrid_apply_vector_device, fimex_amd_interpolation2data_device twice, "
            "on float temporaries allocated once; `chain`) against fimex_amd_regrid_apply_vector_typed_device (`fused`), alternating "
            "launch by launch in one process on the same buffers; per form the median of %d timed repetitions after %d of warm-up, HIP "
            "events.  bytes: fused 2 * pairs * 2 * (N_src + N_out); chain 2 * pairs * (10 * N_src + 10 * N_out); both + the plan and "
            "16 * N_out of (cos, sin) read once.  copy: a device-to-device copy, scaled to the fused form's bytes.  path: what the "
            "entry's dispatch rule chose (2 the kernel on the stored type).  faster_beyond_spread: the medians differ by more than the "
            "two spreads (max - min of the repetitions) together." % (a.reps, a.warmup))
    with open(a.out, "w") as f:
        json.dump({"what": what, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "cases": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
