#!/usr/bin/env python3
"""Records tests/golden/vertical_velocity_answers.npz: mifi_griddistance, mifi_compute_vertical_velocity and
mifi_omega_to_vertical_wind_f answered by the reference's own C code (oracle/_ref/libmifi_ref.so: its unmodified sources, recipe in
oracle/Makefile).

Run from anywhere on a machine where build() found a reference tree:  python scripts/record_vertical_velocity_answers.py
tests/vertical_velocity_ref.py supplies the inputs and the ctypes prototypes; its restatement has no say in what is recorded.  As in
reference_answers.npz the inputs are stored as passed (so that numpy's generators need not stay stable), the outputs as uint32 bit
patterns next to the return codes (tests/golden/vertical_velocity_answers.md).  Keys are "<group>.<case>.<field>":
  grid.<case>      lon, lat -> gridDistX, gridDistY, rc
  velocity.<case>  dx, dy, gridDistX, gridDistY, ap, b, zs, ps, u, v, t -> w, rc
  omega.kind<k>    the level description (kind, nz, p0, ptop and the arrays the kind uses, hPa), p (its float32 field), omega, t -> w, rc
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import vertical_ref as vr  # noqa: E402
import vertical_velocity_ref as vv  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def main():
    ref = vv.reference_lib()
    if ref is None:
        sys.exit("oracle/_ref/libmifi_ref.so is absent: build() found no reference tree")
    out = {}
    for i, (name, nx, ny) in enumerate(vv.RECORDED_GRIDS):
        lon, lat = vv.make_grid(400 + i, nx, ny, lat0=(0.5, 60.0, 89.0)[i % 3])
        gx, gy, rc = ref.griddistance(lon, lat)
        out.update({"grid.%s.lon" % name: lon, "grid.%s.lat" % name: lat, "grid.%s.gridDistX" % name: bits(gx),
                    "grid.%s.gridDistY" % name: bits(gy), "grid.%s.rc" % name: np.int32(rc)})
    for name, _, _, _, _ in vv.RECORDED_VELOCITY:
        c = vv.recorded_velocity_case(name)
        w = ref.vertical_velocity(*vv.velocity_args(c))
        for k in vv.VELOCITY_ARGS:
            out["velocity.%s.%s" % (name, k)] = np.asarray(c[k])
        out["velocity.%s.w" % name] = bits(w)
        out["velocity.%s.rc" % name] = np.int32(vv.OK)
    nx, ny, nz, nt = vv.RECORDED_OMEGA
    for kind in vr.KINDS:
        lv, omega, t = vv.make_omega_case(600 + kind, kind, nx, ny, nz, nt)
        p = vr.level_field(lv, nt, ny, nx)
        w = ref.omega_to_vertical_wind(omega, p, t)
        name = "omega.kind%d." % kind
        out.update({name + "kind": np.int32(kind), name + "nz": np.int32(nz), name + "p0": np.float64(lv.p0), name + "ptop": np.float64(lv.ptop),
                    name + "p": p, name + "omega": omega, name + "t": t, name + "w": bits(w), name + "rc": np.int32(vv.OK)})
        for k in ("axis", "sigma", "a", "ap", "b", "ps", "field"):
            if getattr(lv, k) is not None:
                out[name + k] = getattr(lv, k)
    path = os.path.join(ROOT, "tests", "golden", vv.FIXTURE)
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
