#!/usr/bin/env python3
"""What one *_host call costs, copies and allocations included: the median of 20 calls after 3 warm-ups, at a size where the call is
bound by its allocations (about 1000 elements) and at one where it is bound by its copies (about 4 M elements).  The C entries are
called directly on arrays made once, so that numpy's own allocations stay out of the figure.  One JSON line per entry and size;
--out also writes them to a file.

    bench_host_calls.py --label parent_a --out a.json      (at the parent commit, and once more as parent_b in a second process)
    bench_host_calls.py --label branch --out c.json        (at this code)
    bench_host_calls.py --merge a.json b.json c.json --out profiles/capi_host_calls.json

--merge needs no GPU.  It puts the three runs side by side and applies the rule to every line: this code passes an entry if its
median is no higher than the parent's slower run plus the difference between the parent's two runs."""
import argparse, ctypes, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--label", default="")
ap.add_argument("--merge", nargs=3, metavar=("PARENT_A", "PARENT_B", "BRANCH"))
args = ap.parse_args()


def write(obj):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(obj, fh, indent=1)
            fh.write("\n")


if args.merge:
    a, b, c = ({(l["entry"], l["elements"]): l["median_ms"] for l in json.load(open(p))} for p in args.merge)
    assert a.keys() == b.keys() == c.keys(), "the three runs do not time the same entries"
    rows = []
    for key in a:  # the same arithmetic for every line, project_values' two calls under one label included
        bound = max(a[key], b[key]) + abs(a[key] - b[key])
        rows.append({"entry": key[0], "elements": key[1], "parent_a_ms": round(a[key], 4), "parent_b_ms": round(b[key], 4),
                     "branch_ms": round(c[key], 4), "bound_ms": round(bound, 4), "pass": c[key] <= bound})
        print(json.dumps(rows[-1]))
    write({"protocol": "median of 20 calls after 3 warm-ups; parent twice in separate processes, this code once; one device, one visit",
           "rule": "branch_ms <= max(parent_a_ms, parent_b_ms) + |parent_a_ms - parent_b_ms|", "entries": rows})
    sys.exit(0 if all(r["pass"] for r in rows) else 1)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from fimex_amd import capi as fa
import workloads, bench

lib = fa.load(); fa.set_device(0)
rng = np.random.default_rng(0)
lines = []


def timed(entry, n, call, warmup=3, reps=20):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
    line = {"label": args.label, "entry": entry, "elements": n, "median_ms": float(np.median(ts)) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}
    lines.append(line)
    print(json.dumps(line), flush=True)


def check(rc):
    if rc != fa.OK:
        raise SystemExit(lib.fimex_amd_last_error().decode())


GEO, STERE = b"+proj=latlong +R=6371000", b"+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +a=6371000 +e=0"
for n in (1000, 4 * 1024 * 1024):
    axis = np.linspace(0.0, 99.0, 100)
    pts = rng.uniform(0, 99, n)  # positions are points of the same axis again: no need to restore the input between calls
    timed("points2position_host", n, lambda: check(lib.fimex_amd_points2position_host(fa._dp(pts), n, fa._dp(axis), axis.size, fa.PROJ_AXIS)))

    x, y = np.radians(rng.uniform(-30, 30, n)), np.radians(rng.uniform(50, 80, n))
    def project_values():  # back and forth, so that the values stay in range: the call alone is timed, twice
        check(lib.fimex_amd_project_values_host(GEO, STERE, fa._dp(x), fa._dp(y), n))
        check(lib.fimex_amd_project_values_host(STERE, GEO, fa._dp(x), fa._dp(y), n))
    timed("project_values_host (there and back)", n, project_values)

    top, base, out = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32), np.empty(n, np.float32)
    top[::3] = np.nan
    timed("overlay_host", n, lambda: check(lib.fimex_amd_overlay_host(fa._fp(top), fa._fp(base), fa._fp(out), n)))

    nx, ny, nz = (10, 10, 10) if n == 1000 else (256, 256, 64)
    plane, vol = nx * ny, nx * ny * nz
    gx, gy = np.full(plane, 2500.0, np.float32), np.full(plane, 2500.0, np.float32)
    apc, bc = np.linspace(0.0, 20000.0, nz), np.linspace(0.0, 1.0, nz)
    zs, ps = rng.uniform(0, 500, plane).astype(np.float32), rng.normal(100000, 1500, plane).astype(np.float32)
    u, v, t = (rng.normal(m, 5, vol).astype(np.float32) for m in (5, -3, 270))
    w = np.empty(vol, np.float32)
    timed("vertical_velocity_host", vol, lambda: check(lib.fimex_amd_vertical_velocity_host(
        nx, ny, nz, 1, 2500.0, 2500.0, fa._fp(gx), fa._fp(gy), fa._dp(apc), fa._dp(bc), fa._fp(zs), fa._fp(ps), fa._fp(u), fa._fp(v), fa._fp(t), fa._fp(w))))

    # the two entries whose slab became the most allocations: one became three, two became four
    a1, b1, o1 = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32), np.empty(n, np.float32)
    timed("get_values_1d_f_host", n, lambda: check(lib.fimex_amd_get_values_1d_f_host(fa.BLEND_LINEAR, fa._fp(a1), fa._fp(b1), fa._fp(o1), n, 1.0, 2.0, 1.3)))
    gnx, gny = (40, 25) if n == 1000 else (2048, 2048)
    lon, lat = (np.ascontiguousarray(g.ravel()) for g in np.meshgrid(np.linspace(-20.0, 40.0, gnx), np.linspace(40.0, 75.0, gny)))
    dX, dY = np.empty(gnx * gny, np.float32), np.empty(gnx * gny, np.float32)
    timed("griddistance_host", gnx * gny, lambda: check(lib.fimex_amd_griddistance_host(gnx, gny, fa._dp(lon), fa._dp(lat), fa._fp(dX), fa._fp(dY))))

# the two lines of scripts/bench_host_path.py, in this script's protocol
st = torch.cuda.current_stream().cuda_stream
wl = workloads.BilinearRotatedPole()
plan, px, py = bench.build_plan(fa, torch, wl, fa.BILINEAR, st)
base = wl.base_field()
for nz in (1, 10):
    f = np.ascontiguousarray(np.stack([base + np.float32(0.01 * k) for k in range(nz)]))
    timed("regrid_apply_host nz %d" % nz, f.size, lambda: plan.apply_host(f))
    s16 = (f * 50).astype(np.int16)
    timed("regrid_slice_typed_host (short) nz %d" % nz, f.size, lambda: fa.regrid_slice_typed_host(plan, s16, -32767.0))

write(lines)
