#!/usr/bin/env python3
"""The vertical velocity on model levels (fimex_amd_vertical_velocity_device) on 65 levels, 2000 x 2000, nt = 1, device-resident and
HIP-event timed: median of --launches calls after 3 warm-up calls.  Fields as in scripts/bench_vertical_levels.py (smooth terrain and
surface pressure, T with noise) plus smooth u and v; the grid distances come from fimex_amd_griddistance_device on a perturbed
lon / lat grid and are timed too.  The algorithmic bytes are u, v, T and ps read once and w written once; the scratch of
(nz - 1) * ny * nx doubles that passes between the two kernels is counted separately.  The yardstick is the time of a device-to-device
copy that moves the algorithmic bytes (half read, half written), taken in the same run.  Writes the "results" of
profiles/vertical_velocity_65.json (or --out), keeping the file's other keys, and prints one JSON line per case.

  --cpu-reference   instead: the reference's own mifi_compute_vertical_velocity (oracle/_ref/libmifi_ref.so), one thread, on a
                    500 x 500 x 65 cut of the same fields, on the CPU of the machine this runs on (no GPU needed); written to the
                    "cpu_reference" key of the same file.
usage: python scripts/bench_vertical_velocity.py [--launches 20] [--out FILE] [--cpu-reference]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NX = NY = 2000
NZ = 65
SPACING = 0.0125  # degrees; dx = dy = the same step along a meridian


def hybrid_coefficients():
    """Full levels (ap in Pa, b), index 0 at the top, as means of half levels from p = 0 down to ps."""
    eh = np.arange(NZ + 1, dtype=np.float64) / NZ
    ahh, bhh = 40000.0 * eh * (1 - eh), eh ** 2
    return 0.5 * (ahh[:-1] + ahh[1:]), 0.5 * (bhh[:-1] + bhh[1:])


def fields(xp, nx, ny, f32, f64):
    """The case on an nx x ny cut, with numpy or torch as xp: lon, lat (degrees), zs (m), ps (Pa), t, u, v without the noise of T."""
    jj = xp.arange(ny, dtype=f64)[:, None]
    ii = xp.arange(nx, dtype=f64)[None, :]
    lon = 5.0 + SPACING * ii + 0.2 * SPACING * xp.sin(0.7 * jj + 0.3 * ii)
    lat = 50.0 + SPACING * jj + 0.2 * SPACING * xp.cos(0.5 * ii - 0.2 * jj)
    terrain = 0.5 + 0.5 * xp.sin(0.011 * ii) * xp.cos(0.007 * jj)
    zs = 3000.0 * (1.0 - terrain)
    ps = 60000.0 + 44000.0 * terrain
    eta = ((xp.arange(NZ, dtype=f64) + 0.5) / NZ)[:, None, None]
    t = 210.0 + 80.0 * eta + 0.0 * ii[None] + 2.0 * xp.sin(0.013 * ii + 0.017 * jj)[None]
    u = 25.0 * (1.2 - eta) * xp.cos(0.009 * jj)[None] + 2.0 * xp.sin(0.019 * ii)[None] * (1 + eta)
    v = 10.0 * (1.2 - eta) * xp.sin(0.005 * ii)[None] + 1.5 * xp.cos(0.023 * jj)[None] * (1 + eta)
    return lon, lat, zs, ps, t, u, v


def update(path, key, value):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["script"] = "scripts/bench_vertical_velocity.py"
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def cpu_reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vertical_velocity_ref as vv
    ref = vv.reference_lib()
    if ref is None:
        raise SystemExit("oracle/_ref/libmifi_ref.so is absent: build() found no reference tree")
    nx = ny = 500
    lon, lat, zs, ps, t, u, v = fields(np, nx, ny, np.float32, np.float64)
    gx, gy, _ = ref.griddistance(lon, lat)
    ap, b = hybrid_coefficients()
    d = 6371000.0 * np.pi / 180.0 * SPACING
    a32 = lambda a: np.ascontiguousarray(np.broadcast_to(a, (1,) + a.shape), np.float32)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        w = ref.vertical_velocity(d, d, gx, gy, ap, b, zs.astype(np.float32), a32(ps), a32(u), a32(v), a32(t))
        ts.append(time.perf_counter() - t0)
    r = {"what": "mifi_compute_vertical_velocity of the reference, unmodified, gcc -O2, one thread, measured on the CPU of the build host "
                 "(not on the GPU box)", "nx": nx, "ny": ny, "levels": NZ, "runs": len(ts), "ms_median": 1e3 * float(np.median(ts)),
         "ms_min": 1e3 * float(np.min(ts)), "Mcells_per_s": nx * ny * NZ / float(np.median(ts)) / 1e6,
         "finite_share_of_output": float(np.isfinite(w).mean())}
    print(json.dumps(r), flush=True)
    update(args.out, "cpu_reference", r)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertical_velocity_65.json"))
    ap_.add_argument("--cpu-reference", action="store_true")
    args = ap_.parse_args()
    if args.cpu_reference:
        return cpu_reference(args)
    import torch
    from bench_others import timed
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    plane = NX * NY
    torch.set_default_device("cuda")
    lon, lat, zs, ps, t, u, v = fields(torch, NX, NY, torch.float32, torch.float64)
    torch.set_default_device("cpu")
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    lon, lat = lon.contiguous(), lat.contiguous()
    zs = zs.float().contiguous()
    ps = ps.float().reshape(1, NY, NX).contiguous()
    T = (t.float().reshape(1, NZ, NY, NX) + 2. * torch.randn((1, NZ, NY, NX), device="cuda", generator=gen)).contiguous()
    U, V = u.float().reshape(1, NZ, NY, NX).contiguous(), v.float().reshape(1, NZ, NY, NX).contiguous()
    del t, u, v
    gx, gy = torch.empty((NY, NX), dtype=torch.float32, device="cuda"), torch.empty((NY, NX), dtype=torch.float32, device="cuda")
    out = torch.empty((1, NZ, NY, NX), dtype=torch.float32, device="cuda")
    ap, b = hybrid_coefficients()
    d = 6371000.0 * np.pi / 180.0 * SPACING
    vol, pl = 4 * plane * NZ, 4 * plane
    results = []

    def run(name, call, alg, formula, result, extra):
        src = torch.empty(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        src.zero_()
        copy_ms, copy_min = timed(torch, lambda: dst.copy_(src), reps=args.launches, warm=3)
        del src, dst
        ms, mn = timed(torch, call, reps=args.launches, warm=3)
        torch.cuda.synchronize()
        r = {"case": name, "levels": NZ, "nx": NX, "ny": NY, "nt": 1, "launches": args.launches, "ms_median": ms, "ms_min": mn,
             "algorithmic_bytes": alg, "algorithmic_bytes_formula": formula, "TBps": alg / ms / 1e9,
             "copy_payload_bytes": alg // 2, "copy_ms_median": copy_ms, "copy_ms_min": copy_min, "copy_TBps": alg / copy_ms / 1e9,
             "kernel_over_copy": ms / copy_ms, "finite_share_of_output": float(torch.isfinite(result).float().mean()),
             "output_min": float(result.min()), "output_max": float(result.max()), "device": torch.cuda.get_device_name(0)}
        r.update(extra)
        print(json.dumps(r), flush=True)
        results.append(r)

    run("grid distance", lambda: fa.griddistance_device(NX, NY, lon.data_ptr(), lat.data_ptr(), gx.data_ptr(), gy.data_ptr(), stream=st),
        6 * pl, "nx*ny*(8*2 [lon, lat] + 4*2 [gridDistX, gridDistY])", gx, {})
    out.fill_(-1.0)
    run("vertical velocity on model levels",
        lambda: fa.vertical_velocity_device(NX, NY, 1, d, d, gx.data_ptr(), gy.data_ptr(), ap, b, zs.data_ptr(), ps.data_ptr(), U.data_ptr(),
                                            V.data_ptr(), T.data_ptr(), out.data_ptr(), stream=st),
        4 * vol + pl, "4*nx*ny*(nz [u] + nz [v] + nz [T] + nz [w] + 1 [ps])", out,
        {"scratch_bytes": 8 * plane * (NZ - 1), "scratch": "(nz - 1)*ny*nx doubles (z), written once by the hydrostatic pass and read by the "
                                                           "divergence pass; not part of the algorithmic bytes"})
    update(args.out, "timing", "HIP events around one call, median of the launches after 3 warm-up calls")
    update(args.out, "results", results)


if __name__ == "__main__":
    main()
