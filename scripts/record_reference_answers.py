#!/usr/bin/env python3
"""Records tests/golden/reference_answers.npz: a compact seeded subset of tests/test_oracle_vs_reference.py, answered by the
reference's own C code (oracle/_ref/libmifi_ref.so: its unmodified sources, recipe in oracle/Makefile).

Run from anywhere on a machine where build() found a reference tree:  python scripts/record_reference_answers.py
Imports oracle.ref() and tests/cases.py only; neither the oracle nor a kernel has a say in what is recorded.  Inputs are
stored as passed (so that numpy's generators need not stay stable), outputs as bit patterns with return codes and nChanged.
Positions the reference cannot take (divergences D1, D2 of oracle/fimex_oracle.c) are marked in skip<method> and were never
passed to it; their output cells hold NaN.  tests/reference_answers.py documents the layout.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cases  # noqa: E402
import oracle  # noqa: E402

NEAREST, BILINEAR, BICUBIC = 0, 1, 2
SIGMA, HYBRID_SIGMA, HYBRID_SIGMA_AP = 2, 3, 4  # fimex_amd_vertical_levels kinds


def lround(x):
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.sign(x), 0.0)


def skip_mask(method, px, py, ix, iy):
    """D2: not finite or |coordinate| >= 2^30; for bilinear also D1: nearest/nearest corner with lround(y) == iy."""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(px) & np.isfinite(py) & (np.abs(px) < 2.0 ** 30) & (np.abs(py) < 2.0 ** 30)
    if method != BILINEAR:
        return ~ok
    x, y = np.where(ok, px, 0.0), np.where(ok, py, 0.0)
    xlin = (0 <= np.floor(x)) & (np.floor(x) + 1 < ix)
    ylin = (0 <= np.floor(y)) & (np.floor(y) + 1 < iy)
    return ~ok | (~xlin & (0 <= lround(x)) & (lround(x) < ix) & ~ylin & (lround(y) == iy))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def main():
    ref = oracle.ref()
    if ref is None:
        sys.exit("oracle/_ref/libmifi_ref.so is absent: run build() on a machine with the reference tree")
    out = {}

    def put(name, **fields):
        for k, v in fields.items():
            out["%s.%s" % (name, k)] = np.asarray(v)

    # ---- regrid
    for case, (inX, inY, nz, outX, outY) in (("a", (37, 29, 3, 41, 33)), ("b", (4, 4, 1, 16, 12)), ("c", (97, 61, 2, 23, 19))):
        px, py = cases.backward_positions(inX, inY, outX, outY, seed=300 + inX, special=True)
        f = cases.field(nz, inY, inX, seed=310 + inX, extremes=True)
        fields = {"shape": [inX, inY, nz], "px": px, "py": py, "in": f}
        for method in (NEAREST, BILINEAR, BICUBIC):
            skip = skip_mask(method, px, py, inX, inY)
            o, rc = ref.interpolate_values(method, px, py, f, inX, inY, skip)
            fields.update({"skip%d" % method: skip.astype(np.uint8), "out%d" % method: bits(o), "rc%d" % method: rc})
        put("regrid." + case, **fields)

    # ---- fills
    def slices(fn, f, *args):
        res = [fn(f[z], *args) for z in range(f.shape[0])]
        return {"in": f, "out": bits(np.stack([r[0] for r in res])), "nChanged": [r[1] for r in res], "rc": [r[2] for r in res]}

    small, wide, thin = cases.holes(2, 30, 40, seed=321), cases.holes(1, 61, 97, seed=322), cases.holes(1, 17, 3, seed=323)
    put("fill2d.a", params=[4.0, 1.6, 100], **slices(ref.fill2d, small, 4.0, 1.6, 100))
    put("fill2d.b", params=[1e-9, 1.6, 41], **slices(ref.fill2d, wide, np.float32(1e-9), 1.6, 41))
    put("fill2d.c", params=[0.5, 1.0, 23], **slices(ref.fill2d, thin, 0.5, 1.0, 23))
    put("fill2d.d", params=[4.0, 1.9, 3], **slices(ref.fill2d, small, 4.0, 1.9, 3))
    put("creepfill2d.a", params=[20, 2], **slices(ref.creepfill2d, small, 20, 2))
    put("creepfill2d.b", params=[3, 0], **slices(ref.creepfill2d, wide, 3, 0))
    put("creepfill2d.c", params=[2, -1], **slices(ref.creepfill2d, cases.holes(1, 40, 50, seed=5), 2, -1))
    put("creepfill2d.d", params=[1, 1], **slices(ref.creepfill2d, thin, 1, 1))
    put("creepfillval2d.a", params=[5, 2, 271.25], **slices(ref.creepfillval2d, small, 271.25, 5, 2))
    put("creepfillval2d.b", params=[2, 7, 271.25], **slices(ref.creepfillval2d, wide, 271.25, 2, 7))

    # ---- rotation
    ox, oy, oz = 41, 33, 2
    m = cases.rotation_matrix(ox, oy, seed=330)
    u, v = cases.field(oz, oy, ox, seed=331), cases.field(oz, oy, ox, seed=332) - 280
    ang = np.random.default_rng(333).uniform(-30, 400, (oz, oy, ox)).astype(np.float32)
    wu, wv, rc = ref.vector_reproject_values(m, u, v, ox, oy)
    wa, rca = ref.vector_reproject_direction(m, ang, ox, oy)
    put("rotation.a", shape=[ox, oy, oz], matrix=m, u=u, v=v, angles=ang, u_out=bits(wu), v_out=bits(wv), angles_out=bits(wa), rc=[rc, rca])

    # ---- axis positions
    rng = np.random.default_rng(340)
    for case, axis, typ in (("asc", np.linspace(-5, 5, 41), 0), ("desc", np.linspace(9, -3, 25), 0),
                            ("lon_pm180", np.radians(np.arange(-180, 180, 1.0)), 1), ("lon_0_360", np.radians(np.arange(0, 360, 0.5)), 1),
                            ("lat_desc", np.radians(np.linspace(80, -80, 321)), 2)):
        p = rng.uniform(-8, 8, 600)
        p[::37] = axis[rng.integers(0, axis.size, p[::37].size)]
        p[5:12] = np.nan, np.inf, -np.inf, axis[0], axis[-1], np.pi, -np.pi
        o, rc = ref.points2position(p, axis, typ)
        put("points2position." + case, points=p, axis=axis, axis_type=typ, out=bits(o), rc=rc)

    # ---- 1-D blends
    A, B = cases.field(1, 19, 23, seed=350, nan_frac=0.05)[0], cases.field(1, 19, 23, seed=351, nan_frac=0.05)[0]
    abxs = [(1., 2., 1.5), (0., 1., 2.5), (1000., 100., 500.), (0., 1., -1.5), (3., 7., 3.0000001), (1., 1., .5)]
    kabx = [(k, a, b, x) for k in range(7) for a, b, x in abxs]
    res = [ref.get_values_1d(int(k), A, B, a, b, x) for k, a, b, x in kabx]
    resd = [ref.get_values_linear_d(A.astype(np.float64), B.astype(np.float64), a, b, x) for a, b, x in abxs]
    put("blend.a", A=A, B=B, kabx=np.array(kabx, np.float64), out=bits(np.stack([r[0] for r in res])), rc=[r[1] for r in res],
        abx_d=np.array(abxs, np.float64), out_d=bits(np.stack([r[0] for r in resd])), rc_d=[r[1] for r in resd])

    # ---- fill value <-> NaN
    rng = np.random.default_rng(360)
    a = rng.normal(0, 1, 2003).astype(np.float32)
    for v in (9.96921e36, -32767.0, np.nan, np.inf, 0.0, -0.0, 1e-42):
        a[rng.choice(a.size, 40, replace=False)] = np.float32(v)
    bad = np.array([9.96921e36, -32767.0, 0.0, -0.0, np.inf, 1e-42, np.nan], np.float32)
    put("badvalue.a", **{"in": a, "bad": bits(bad), "bad2nan": bits(np.stack([ref.bad2nan(a, b)[0] for b in bad])),
                         "nan2bad": bits(np.stack([ref.nan2bad(a, b)[0] for b in bad]))})

    # ---- level pressures, one call per column
    rng = np.random.default_rng(370)
    nx, ny, nt, nz = 5, 4, 2, 9
    ps = rng.uniform(600, 1040, (nt, ny, nx)).astype(np.float32)
    ps[0, 1, 2] = np.nan
    c = rng.uniform(0, 1, nz)
    for case, kind, name, scalars, arrays in (("sigma", SIGMA, "mifi_atmosphere_sigma_pressure", dict(ptop=5.0), dict(sigma=c)),
                                              ("hybrid", HYBRID_SIGMA, "mifi_atmosphere_hybrid_sigma_pressure", dict(p0=1000.0), dict(a=0.3 * c, b=c * c)),
                                              ("ap", HYBRID_SIGMA_AP, "mifi_atmosphere_hybrid_sigma_ap_pressure", {}, dict(ap=300 * c, b=c * c))):
        o = np.empty((nt, nz, ny, nx))
        for t in range(nt):
            for j in range(ny):
                for i in range(nx):
                    col, rc = ref.level_pressure(name, *scalars.values(), float(ps[t, j, i]), *arrays.values())
                    assert rc == 1
                    o[t, :, j, i] = col
        put("levels." + case, kind=kind, nz=nz, p0=scalars.get("p0", 0.0), ptop=scalars.get("ptop", 0.0), ps=ps, out=bits(o), **arrays)

    path = os.path.join(ROOT, "tests", "golden", "reference_answers.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
