#!/usr/bin/env python3
"""A vector pair regridded and rotated: the three launches (regrid u, regrid v, rotate) against the fused entry
(fimex_amd_regrid_apply_vector_device), in one process and on the same buffers, alternating launch by launch.

Geometries: the headline plan of bench.py (4000 x 3000 -> 2000 x 2000) with 100 pairs, and shorter batches of it down to the
dispatch threshold; the plan of BASELINE configs[4] (scripts/bench_c5_chain.py: 3000 x 3000 polar stereographic -> 3000 x 3000
lat/lon) with 16 pairs.  Nearest and bilinear; bilinear also on the plan's second workgroup shape (tuning build,
FIMEX_AMD_STAGE2_USE_ALT=1).  Per case: the fused result is compared with the chain's bit for bit, then after warm-up the median of
REPS timed repetitions of each form from HIP events; algorithmic bytes of both, TB/s, the ratio chain / fused, and a device copy
of the fused form's bytes for scale.

usage: python scripts/bench_vector_regrid.py [--reps 20] [--warmup 3] [--out profiles/vector_regrid.json]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_regrid.json"))
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed repetitions"
    import torch
    from fimex_amd import capi as fa
    import bench, workloads
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    ev = lambda: torch.cuda.Event(enable_timing=True)
    results = []

    def same_bits(x, y):
        return bool(((x.view(torch.int32) == y.view(torch.int32)) | (x.isnan() & y.isnan())).all().item())

    def smooth_matrix(ox, oy):  # (cos, sin, -sin, phi) of a smooth angle field: the kernels' time does not depend on the values
        j, i = np.meshgrid(np.arange(oy), np.arange(ox), indexing="ij")
        phi = (0.9 * np.sin(0.005 * i) + 0.7 * np.cos(0.003 * j)).ravel()
        return np.stack([np.cos(phi), np.sin(phi), -np.sin(phi), phi], axis=1).ravel()

    def run(name, geometry, method, plan, vec, d_u, d_v, nz, note=None):
        inL, outL = plan.inX * plan.inY, plan.outX * plan.outY
        bufs = [torch.empty((nz, plan.outY, plan.outX), dtype=torch.float32, device="cuda") for _ in range(4)]
        cu, cv, fu, fv = bufs
        ptr = [b.data_ptr() for b in bufs]

        def chain():
            plan.apply_device(d_u.data_ptr(), nz, ptr[0], st)
            plan.apply_device(d_v.data_ptr(), nz, ptr[1], st)
            vec.reproject_values_device(ptr[0], ptr[1], nz, st)

        def fused():
            return plan.apply_vector_device(vec, d_u.data_ptr(), d_v.data_ptr(), nz, ptr[2], ptr[3], st)

        chain(); path = fused(); torch.cuda.synchronize()
        ok = same_bits(cu, fu) and same_bits(cv, fv)
        assert ok, "%s: the fused result differs from the chain's" % name
        t = {"chain": [], "fused": [], "copy": []}
        info = plan.info()
        plan_bytes, matrix_bytes = info["planBytes"], 16 * outL
        bytes_fused = 2 * nz * 4 * (inL + outL) + plan_bytes + matrix_bytes
        bytes_chain = 2 * nz * 4 * (inL + outL) + 2 * plan_bytes + 16 * nz * outL + matrix_bytes
        src = d_u.view(-1)[: bytes_fused // 8]  # bytes_fused / 2 bytes of floats
        dst = torch.empty_like(src)
        for rep in range(a.warmup + a.reps):
            for form, fn in (("chain", chain), ("fused", fused), ("copy", lambda: dst.copy_(src))):
                e0, e1 = ev(), ev()
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    t[form].append(e0.elapsed_time(e1))
        ms = {k: float(np.median(v)) for k, v in t.items()}
        ms["copy_scaled_to_fused_bytes"] = ms["copy"] * bytes_fused / (2 * src.numel() * 4)
        rec = {"case": name, "geometry": geometry, "method": method, "pairs": nz, "path": path, "same_bits_as_chain": ok,
               "ms": ms, "ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in t.items()},  # copy: as many of the bytes as the u batch holds
               "bytes": {"chain": bytes_chain, "fused": bytes_fused, "plan": plan_bytes, "matrix": matrix_bytes, "copy": 2 * src.numel() * 4},
               "TB_per_s": {"chain": bytes_chain / ms["chain"] / 1e9, "fused": bytes_fused / ms["fused"] / 1e9,
                            "copy": 2 * src.numel() * 4 / ms["copy"] / 1e9},
               "chain_over_fused": ms["chain"] / ms["fused"],
               "plan": {k: info[k] for k in ("stagedCells", "tileW", "tileH", "undefinedCells")}}
        if note:
            rec["note"] = note
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del bufs, cu, cv, fu, fv, src, dst

    # ---- the headline geometry
    wl = workloads.BilinearRotatedPole()
    d_u = bench.make_slices(torch, wl.base_field(), 100)
    d_v = bench.make_slices(torch, wl.base_field() - 280, 100)
    vec = fa.VectorPlan(smooth_matrix(wl.outX, wl.outY), wl.outX, wl.outY)
    headline = "%dx%d -> %dx%d (bench.py headline)" % (wl.inX, wl.inY, wl.outX, wl.outY)
    for method, mname in ((fa.NEAREST_NEIGHBOR, "nearest"), (fa.BILINEAR, "bilinear")):
        plan, _, _ = bench.build_plan(fa, torch, wl, method, st)
        for nz in (100, 25, 8, 4):
            run("headline_%s_%dpairs" % (mname, nz), headline, mname, plan, vec, d_u, d_v, nz)
        plan.close()
    # the second workgroup shape of the bilinear plan (512 threads): the tuning build reads the switch at every launch
    fa.use_tuning_build(True)
    os.environ["FIMEX_AMD_STAGE2_USE_ALT"] = "1"
    plan, _, _ = bench.build_plan(fa, torch, wl, fa.BILINEAR, st)
    vec_t = fa.VectorPlan(smooth_matrix(wl.outX, wl.outY), wl.outX, wl.outY)
    for nz in (100, 25):
        run("headline_bilinear_512threads_%dpairs" % nz, headline, "bilinear", plan, vec_t, d_u, d_v, nz,
            note="tuning build, FIMEX_AMD_STAGE2_USE_ALT=1: both forms on the plan's 512-thread shape")
    plan.close(); vec_t.close()
    del os.environ["FIMEX_AMD_STAGE2_USE_ALT"]
    fa.use_tuning_build(False)
    del d_u, d_v
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
    d_u = torch.stack([u0 * (1 + 0.01 * k) for k in range(nz)]); d_v = torch.stack([v0 * (1 + 0.01 * k) for k in range(nz)])
    del xx, yy, ang
    for method, mname in ((fa.NEAREST_NEIGHBOR, "nearest"), (fa.BILINEAR, "bilinear")):
        fa.project_axes_device(geo, stere, np.radians(lon), np.radians(lat), d_px.data_ptr(), d_py.data_ptr(), st)
        fa.points2position_device(d_px.data_ptr(), d_px.numel(), sx, fa.PROJ_AXIS, st)
        fa.points2position_device(d_py.data_ptr(), d_py.numel(), sy, fa.PROJ_AXIS, st)
        plan = fa.RegridPlan.from_device(method, d_px.data_ptr(), d_py.data_ptr(), d_px.numel(), n, n, ox, oy, st)
        run("c5_%s_16pairs" % mname, "3000x3000 polar stereographic -> 3000x3000 lat/lon (BASELINE configs[4])", mname, plan, vec, d_u, d_v, nz)
        plan.close()
    what = ("A vector pair regridded and rotated on one MI355X, device resident: the three launches (regrid u, regrid v, rotate; `chain`) "
            "against fimex_amd_regrid_apply_vector_device (`fused`), alternating launch by launch in one process on the same buffers; "
            "per form the median of %d timed repetitions after %d of warm-up, HIP events.  bytes: 2 * pairs * 4 * (N_src + N_out) for "
            "the regrids, + 16 * pairs * N_out for the rotation pass of the chain, + the plan (twice in the chain) and 16 * N_out of "
            "(cos, sin) read once.  copy: a device-to-device copy that moves the fused form's bytes.  path: what the entry's dispatch "
            "rule chose (1 fused, 0 the chain itself)." % (a.reps, a.warmup))
    with open(a.out, "w") as f:
        json.dump({"what": what, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "cases": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
