#!/usr/bin/env python3
"""Times the fills on [nz][ny][nx] slices with land-mask like holes (device resident, wall time of the call), one JSON line per
measurement.  usage: python scripts/bench_fills.py [--mode MODE] [numbers ...]

  kernels      the fill kernels, systolic and wavefront                      [nx ny nz]
  fixed        per-call cost of fill2d: the scan-order sums (SUM_ALGO)       [algo ...]
  batch        seconds per sweep over batch sizes, systolic and wavefront
  geometry     the two band geometries over batch sizes (where FILL_WIDE_NZ belongs), then whole calls per geometry
  multi        small batches: workgroups per slice and their shape           [nz ...]
  scaling      sweep time against the number of 64-row bands
  shape        one slice: time per sweep against bands and row length
  creep-skip   creepfill2d on a field without salt-and-pepper holes: idle chunks passed over (CREEP_SKIP)
  creep-small  creepfill2d on small fields with one undefined corner: several workgroups per slice against one

All modes but scaling and shape load the tuning build, which reads the FIMEX_AMD_<NAME> switches."""
import argparse, contextlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from fimex_amd import capi as fa
import cases

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--mode", default="kernels", choices=["kernels", "fixed", "batch", "geometry", "multi", "scaling", "shape", "creep-skip", "creep-small"])
ap.add_argument("numbers", nargs="*")
args = ap.parse_args()
fa.use_tuning_build(args.mode not in ("scaling", "shape"))
fa.load(); fa.set_device(0)
st = torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def switches(env):
    for k, v in env.items(): os.environ["FIMEX_AMD_" + k] = v
    try:
        yield
    finally:
        for k in env: os.environ.pop("FIMEX_AMD_" + k, None)


def timed(call, d0, reps):
    """seconds of each of `reps` calls on a fresh copy of d0, and the last copy"""
    ts = []
    for _ in range(reps):
        d = d0.clone(); torch.cuda.synchronize()
        t0 = time.perf_counter(); call(d); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return ts, d


def holes(nx, ny, nz):
    h = cases.holes(1, ny, nx, seed=4, frac=0.3)[0]
    return torch.from_numpy(h[None]).cuda().repeat(nz, 1, 1).contiguous()


def fill2d(nx, ny, nz, crit, loops):
    return lambda d: fa.fill2d_device(d.data_ptr(), nx, ny, nz, crit, 1.6, loops, st)


def creep(nx, ny, nz):
    return lambda d: fa.creepfill2d_device(d.data_ptr(), nx, ny, nz, 20, 2, st)


def out(**row):
    print(json.dumps(row), flush=True)


def per_sweep(nx, ny, nz, d0, few, many, reps):
    """(seconds per sweep, seconds of the call with `few` sweeps) of fill2d without early exit"""
    res = {loops: min(timed(fill2d(nx, ny, nz, 1e-12, loops), d0, reps)[0]) for loops in (few, many)}
    return (res[many] - res[few]) / (many - few), res[few]


def kernels():
    nx, ny, nz = (int(v) for v in args.numbers[:3]) if len(args.numbers) >= 3 else (3000, 3000, 16)
    d0 = holes(nx, ny, nz)
    for name, call, env in (("fill2d(4,1.6,100) systolic", fill2d(nx, ny, nz, 4.0, 100), {}),
                            ("fill2d(4,1.6,100) wavefront", fill2d(nx, ny, nz, 4.0, 100), {"FILL_V2": "0"}),
                            ("fill2d(1e-9,1.6,100) systolic, no early exit", fill2d(nx, ny, nz, 1e-9, 100), {}),
                            ("creepfill2d(20,2)", creep(nx, ny, nz), {}),
                            ("creepfill2d(20,2) wavefront", creep(nx, ny, nz), {"CREEP_V2": "0"})):
        with switches(env):
            ts = timed(call, d0, 3)[0]
        out(kernel=name, nx=nx, ny=ny, nz=nz, seconds_min=min(ts), seconds_all=ts, Mcells_per_s=nz * nx * ny / min(ts) / 1e6)


def fixed():
    nx = ny = 3000
    d0 = holes(nx, ny, 4)
    for algo in args.numbers or ["0", "1", "2"]:
        os.environ["FIMEX_AMD_SUM_ALGO"] = algo
        out(sum_algo=int(algo), ms_one_sweep_call=min(timed(fill2d(nx, ny, 4, 1e-12, 1), d0, 3)[0]) * 1e3)
    x = d0[0].contiguous().view(-1)
    for algo in (0, 1, 2):
        for mode, avg in ((0, 0.0), (1, 280.0)):
            best = 1e9
            for _ in range(3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fa.scan_sum_device(x.data_ptr(), x.numel(), mode, avg, algo, st)
                best = min(best, time.perf_counter() - t0)
            out(scan_sum_algo=algo, mode=mode, n=x.numel(), ms=best * 1e3)


def batch():
    nx = ny = 3000
    for nz in (1, 16, 64, 200):
        d0 = holes(nx, ny, nz)
        for v2 in ("1", "0"):
            os.environ["FIMEX_AMD_FILL_V2"] = v2
            per, few = per_sweep(nx, ny, nz, d0, 6, 16, 1)
            out(nz=nz, kernel="systolic" if v2 == "1" else "wavefront", ms_per_sweep=per * 1e3, fixed_ms=(few - 6 * per) * 1e3,
                Mcell_updates_per_s=nz * nx * ny / per / 1e6)
        del d0


def geometry():
    nx = ny = 3000
    for nz in (8, 16, 24, 32, 48, 64, 96):
        d0 = holes(nx, ny, nz)
        row = {"nz": nz}
        for geom, name in (("1", "16x16"), ("2", "8x32")):
            with switches({"FILL_GEOMETRY": geom}):
                row["ms_per_sweep_" + name] = per_sweep(nx, ny, nz, d0, 6, 16, 2)[0] * 1e3
        out(**row)
        del d0
    for nz in (200, 64, 32):
        d0 = holes(nx, ny, nz)
        for env in ({"FILL_GEOMETRY": "1"}, {"FILL_GEOMETRY": "2"}, {}):
            with switches(env):
                out(nz=nz, env=env, fill2d_s=min(timed(fill2d(nx, ny, nz, 1e-9, 100), d0, 2)[0]), creepfill_s=min(timed(creep(nx, ny, nz), d0, 2)[0]))
        del d0


def multi():
    nx = ny = 3000
    for nz in [int(v) for v in args.numbers] or [16, 1]:
        d0 = holes(nx, ny, nz)
        for env in ({"FILL_MULTI": "0"}, {"FILL_MULTI_WAVES": "4", "FILL_MULTI_CH": "16"}, {"FILL_MULTI_WAVES": "4", "FILL_MULTI_CH": "32"},
                    {"FILL_MULTI_WAVES": "8", "FILL_MULTI_CH": "16"}, {"FILL_MULTI_WAVES": "8", "FILL_MULTI_CH": "32"}, {"FILL_MULTI_WAVES": "16"}):
            with switches(env):
                out(nz=nz, env=env, seconds_min=min(timed(fill2d(nx, ny, nz, 1e-9, 100), d0, 3)[0]))


def scaling():
    nx = 3000
    for ny in (66, 130, 258, 1026, 2050, 3000):
        per, few = per_sweep(nx, ny, 1, holes(nx, ny, 1), 20, 60, 2)
        bands = (ny - 2 + 63) // 64
        out(ny=ny, bands=bands, ms_per_sweep=per * 1e3, fixed_ms=(few - 20 * per) * 1e3,
            us_per_step_if_serial_bands=per * 1e6 / (((bands + 15) // 16) * (nx + 61)))


def shape():
    for nx, ny in ((3000, 130), (3000, 258), (3000, 514), (3000, 1026), (3000, 3000), (1000, 3000), (6000, 1026), (300, 3000)):
        ts = timed(fill2d(nx, ny, 1, 1e-9, 100), holes(nx, ny, 1), 3)[0]
        out(nx=nx, ny=ny, bands=(ny - 2 + 63) // 64, ms_per_sweep=min(ts) * 10)


def creep_skip():
    nx = ny = 3000
    rng = np.random.default_rng(4)
    f = cases.field(1, ny, nx, 4, nan_frac=0.0, extremes=False)[0]
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    mask = np.zeros((ny, nx), bool)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, ny), rng.uniform(0, nx), rng.uniform(0.05, 0.2) * nx
        mask |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    f[mask] = np.nan
    for nz in (16, 200):
        d0 = torch.from_numpy(f[None]).cuda().repeat(nz, 1, 1).contiguous()
        res = {}
        for skip in ("1", "0"):
            os.environ["FIMEX_AMD_CREEP_SKIP"] = skip
            ts, d = timed(creep(nx, ny, nz), d0, 3)
            res[skip] = (min(ts), d.cpu().numpy()[0])
        assert np.array_equal(res["1"][1].view(np.uint32), res["0"][1].view(np.uint32))
        out(nz=nz, hole_fraction=float(mask.mean()), seconds_skip=res["1"][0], seconds_noskip=res["0"][0])
        del d0


def creep_small():
    os.environ["FIMEX_AMD_CREEP_RECTS"] = "0"
    for (nx, ny, nz) in ((212, 550, 32), (536, 450, 16), (212, 550, 8), (1000, 1000, 16)):
        yy, xx = np.mgrid[0:ny, 0:nx]
        f = (280 + np.sin(xx * 0.01) + np.cos(yy * 0.02)).astype(np.float32)
        f[(yy * (nx / ny) + xx) < nx * 0.8] = np.nan
        h = torch.from_numpy(np.stack([f] * nz)).cuda()
        d = h.clone()
        for multi in ("1", "0"):
            os.environ["FIMEX_AMD_FILL_MULTI"] = multi
            ts = []
            for r in range(4):  # device time between two events; the first call is left out
                d.copy_(h); torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); creep(nx, ny, nz)(d); b.record(); torch.cuda.synchronize()
                if r: ts.append(a.elapsed_time(b))
            out(nx=nx, ny=ny, nz=nz, multi=multi, ms=round(float(np.median(ts)), 3))


{"kernels": kernels, "fixed": fixed, "batch": batch, "geometry": geometry, "multi": multi, "scaling": scaling, "shape": shape,
 "creep-skip": creep_skip, "creep-small": creep_small}[args.mode]()
