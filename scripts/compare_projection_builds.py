#!/usr/bin/env python3
"""Compares the projection kernels of two builds of the library: the same bits, and the same time on the benchmark geometry.

  compare_projection_builds.py --parent DIR [--rounds 5] [--out profiles/projection_split_parent_vs_new.json]

DIR holds libfimex_amd.so built from the commit to compare with; the other side is the library of this tree.  The driver
(compare_builds.py) alternates the sides, one fresh process per side and round, and stops at the first that does not end normally.
Bits (sha256 of the output bytes): every string of ALL and ELLIPSOIDAL of tests/projection_cases.py forward from geographic and back
at 4 096 seeded points, the five datum pairs, UTM 33 in km from Oslo's meridian, project_axes ROT -> STERE on 301 x 200, the rotation
matrix through its three entry points on 64 x 48, and the bounding-box flags of coordTest.nc's first box.  Time (and bits): on the
benchmark geometry's 4 M cells project_axes_device and the rotation matrix as scripts/bench_planbuild.py times them, and
project_values_device of as many points into UTM 33.
"""
import argparse, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compare_builds  # beside this script

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
compare_builds.add_arguments(ap, os.path.join(ROOT, "profiles", "projection_split_parent_vs_new.json"))
args = ap.parse_args()


def worker():
    import numpy as np
    import torch
    from fimex_amd import capi as fa
    import workloads
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import projection_cases as pc
    from extract_ref import BOXES, coordtest
    if args.lib:
        fa.LIB_PATH = os.path.join(args.lib, "libfimex_amd.so")
    lib = fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream

    def sha(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    def bits(name, *arrays):
        print(json.dumps({"case": name, "sha256": sha(*arrays)}), flush=True)

    def there_and_back(name, src, dst, lon, lat):
        x, y = fa.project_values_host(src, dst, lon, lat)
        bx, by = fa.project_values_host(dst, src, x, y)
        bits(name, x, y, bx, by)

    for i, dst in enumerate(pc.ALL):
        there_and_back("sphere_%02d %s" % (i, dst), pc.GEO, dst, *pc.spherical_points(dst, 4096))
    for i, dst in enumerate(pc.ELLIPSOIDAL):
        there_and_back("ellipsoid_%02d %s" % (i, dst), pc.GEO_W, dst, *pc.ellipsoidal_points(dst, 4096))
    rng = np.random.default_rng(3)
    lon, lat = np.radians(rng.uniform(-10, 30, 4096)), np.radians(rng.uniform(35, 70, 4096))
    for i, (src, dst) in enumerate(pc.DATUM_PAIRS):
        there_and_back("datum_%d" % i, src, dst, lon, lat)
    there_and_back("utm33_km_oslo", pc.GEO_W, pc.UTM33 + " +units=km +pm=oslo", np.radians(rng.uniform(2, 28, 4096)), np.radians(rng.uniform(45, 80, 4096)))
    bits("project_axes_rot_stere_301x200", *fa.project_axes_host(pc.ROT, pc.STERE, np.radians(np.linspace(-12, 12, 301)), np.radians(np.linspace(15, 45, 200))))
    bits("matrix_axes_64x48", fa.get_vector_reproject_matrix_host(pc.STERE, pc.GEO, np.linspace(-25, 25, 64), np.linspace(52, 78, 48), fa.LONGITUDE, fa.LATITUDE))
    xx, yy = np.meshgrid(np.linspace(-8e5, 8e5, 64), np.linspace(-6e5, 7e5, 48))
    bits("matrix_field_64x48", fa.get_vector_reproject_matrix_field_host(pc.STERE_OBL, pc.GEO, xx, yy))
    plon, plat = np.meshgrid(np.radians(np.linspace(-20, 40, 64)), np.radians(np.linspace(45, 80, 48)))
    bits("matrix_points_64x48", fa.get_vector_reproject_matrix_points_host(pc.STERE, pc.GEO, True, plon, plat))
    c = coordtest()
    bits("bounding_box_coordtest", *fa.extract_bounding_box_host(c["proj"], "+proj=latlong +R=6.371e6", c["x"], c["y"], *BOXES[0][0]))

    wl = workloads.BilinearRotatedPole()
    n = wl.outX * wl.outY
    tx, ty = np.radians(wl.target_axes_deg()[0]), np.radians(wl.target_axes_deg()[1])
    d = torch.empty(2 * n, dtype=torch.float64, device="cuda")
    m = torch.empty(4 * n, dtype=torch.float64, device="cuda")

    def timed(name, launch, d_out, before=lambda: None):
        ts = []
        for i in range(5):  # two to warm up
            before(); torch.cuda.synchronize()
            t0 = time.perf_counter(); launch(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        print(json.dumps({"case": name, "seconds": ts[2:], "sha256": sha(d_out.cpu().numpy())}), flush=True)

    timed("time_project_axes_4M", lambda: fa.project_axes_device(wl.target_proj, wl.source_proj, tx, ty, d.data_ptr(), d.data_ptr() + 8 * n, st), d)
    timed("time_vector_matrix_4M", lambda: fa.get_vector_reproject_matrix_device(wl.source_proj, wl.target_proj, np.degrees(tx), np.degrees(ty), fa.LONGITUDE,
                                                                                 fa.LATITUDE, m.data_ptr(), st), m)
    pts = torch.from_numpy(np.concatenate([np.radians(rng.uniform(3, 27, n)), np.radians(rng.uniform(-70, 84, n))])).cuda()

    def project_values():
        fa._check(lib.fimex_amd_project_values_device(pc.GEO_W.encode(), pc.UTM33.encode(), d.data_ptr(), d.data_ptr() + 8 * n, n, st))
    timed("time_project_values_utm33_4M", project_values, d, before=lambda: d.copy_(pts))


WHAT = ("The projection kernels: bits of every projection string forward and back, the datum shifts, units and prime meridian, project_axes, the "
        "rotation matrix's three entry points and the bounding-box flags; time of project_axes_device, the rotation matrix and "
        "project_values_device into UTM 33 on the benchmark geometry's 4 M cells (host clock around the call and a device synchronisation).")

worker() if args.worker else compare_builds.drive(__file__, args, WHAT)
