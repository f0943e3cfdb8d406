"""tests/vertical_levels_ref.py, the CPU yardstick of the vertical level converters, against the reference's known answers
(tests/golden/vertical_transform_kats.json: the functions of src/vertical_coordinate_transformations.c compiled unmodified and
run on seeded inputs) and against itself (the vectorised integration loop equals the per-cell one bit for bit).  CPU only.
"""
import json
import os

import numpy as np

import vertical_levels_ref as vl
import vertical_ref as vr

KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vertical_transform_kats.json")


def _load(name):
    """-> (list of input arrays, output array) of one function, decoded from the bit patterns."""
    fn = json.load(open(KATS))["functions"][name]
    types = [a.split(":")[1] for a in fn["arguments"]] + [fn["result"]]
    cols = list(zip(*fn["cases"]))
    assert len(cols) == len(types) and len(cols[0]) >= 200
    out = []
    for ty, col in zip(types, cols):
        if ty == "f32":
            assert all(len(c) == 8 for c in col)
            out.append(np.array([int(c, 16) for c in col], np.uint32).view(np.float32))
        else:
            assert all(len(c) == 16 for c in col)
            out.append(np.array([int(c, 16) for c in col], np.uint64).view(np.float64))
    return out[:-1], out[-1]


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _ulps_f32(a, b):
    """Distance in float32 steps between two finite float32 arrays."""
    key = lambda v: np.where(_bits(v).astype(np.int64) & 0x80000000, -(_bits(v).astype(np.int64) & 0x7fffffff), _bits(v).astype(np.int64))
    return np.abs(key(a) - key(b))


def test_fixture_holds_the_cases_the_functions_need():
    (q, T), _ = _load("mifi_virtual_temperature")
    assert np.count_nonzero(q == 0) >= 10
    (pl, ph, _), lt = _load("mifi_barometric_layer_thickness")
    assert np.count_nonzero(pl == ph) >= 10 and np.all(lt[pl == ph] == 0)
    for name in ("mifi_ocean_s_g1_z", "mifi_ocean_s_g2_z"):
        (h, hc, zeta, _, _), _ = _load(name)
        assert np.any(zeta > 0) and np.any(zeta < 0) and np.any(zeta == 0)
        assert np.count_nonzero((h != hc) & (np.abs(h - hc) <= 1e-5 * hc)) >= 10 and np.any(h == hc)


def test_virtual_temperature_is_bit_identical():
    (q, T), want = _load("mifi_virtual_temperature")
    got = vl.virtual_temperature(q, T)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))


def test_ocean_formulas_are_bit_identical():
    for name, fn in (("mifi_ocean_s_g1_z", vl.ocean_s_g1_z), ("mifi_ocean_s_g2_z", vl.ocean_s_g2_z)):
        (h, hc, zeta, sigma, C), want = _load(name)
        got = fn(h, hc, zeta, sigma, C)
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want)), name
        one = np.array([fn(float(a), float(b), float(c), float(d), float(e)) for a, b, c, d, e in zip(h, hc, zeta, sigma, C)])
        assert np.array_equal(_bits(one), _bits(want)), name + " (scalars)"


def test_functions_through_log_and_exp_are_within_one_float_ulp():
    """numpy's log / exp need not be the C library's: within one float32 step of the reference; the share of identical bits is
    printed.  With the C library's log (the one the integration uses) the layer thickness is bit-identical."""
    (pl, ph, T), want = _load("mifi_barometric_layer_thickness")
    got = vl.layer_thickness(pl, ph, T)
    assert np.all(_ulps_f32(got, want) <= 1)
    print("layer thickness: %.2f %% bit-identical with numpy's log" % (100.0 * np.mean(_bits(got) == _bits(want))))
    assert np.array_equal(_bits(vl.layer_thickness(pl, ph, T, log=vl.c_log)), _bits(want))
    for name, fn in (("mifi_barometric_standard_altitude", vl.standard_altitude), ("mifi_barometric_standard_pressure", vl.standard_pressure)):
        (x,), want = _load(name)
        got = fn(x)
        assert got.dtype == np.float64
        assert np.all(_ulps_f32(got.astype(np.float32), want.astype(np.float32)) <= 1), name
        print("%s: %.2f %% bit-identical as doubles, %.2f %% as floats" % (
            name, 100.0 * np.mean(_bits(got) == _bits(want)), 100.0 * np.mean(_bits(got.astype(np.float32)) == _bits(want.astype(np.float32)))))


def test_vectorised_integration_equals_the_per_cell_loop():
    for seed, surface_first, humidity, nan_frac in ((1, True, True, 0.0), (2, False, True, 0.02), (3, True, False, 0.02), (4, False, False, 0.0)):
        nx, ny, nt, nz = 7, 5, 2, 65
        lv, T, q, sap, sgp = vl.make_atmosphere(seed, vr.HYBRID_SIGMA_AP, nx, ny, nt, nz, surface_first, nan_frac)
        if not humidity:
            q = None
        if nan_frac:
            sap[0, 1, 2] = np.nan  # lv.ps is this array
        p = vr.level_field(lv, nt, ny, nx)
        for flag in (vl.AUTO, int(surface_first)):
            a, spread = vl.integrate(p, T, q, sap, sgp, flag)
            assert vl.surface_first(p, flag) == surface_first
            for t in range(nt):
                for j in range(ny):
                    for i in range(nx):
                        ca, cs = vl.integrate_cell(p[t, :, j, i], T[t, :, j, i], None if q is None else q[t, :, j, i], sap[t, j, i], sgp[t, j, i],
                                                   surface_first)
                        assert np.array_equal(_bits(np.array(ca)), _bits(a[t, :, j, i])), (seed, t, j, i)
                        assert np.array_equal(_bits(np.array(cs)), _bits(spread[t, :, j, i])), (seed, t, j, i)
        fin = np.isfinite(a)
        assert fin.mean() > 0.3 and a[fin].min() > 0 and a[fin].max() < 80000
        if nan_frac:
            assert np.all(np.isnan(a[0, :, 1, 2]))  # a NaN surface pressure: the whole column
            # a NaN in T makes the column NaN from that level upward
            order = slice(None) if surface_first else slice(None, None, -1)
            assert np.all(np.diff(np.isnan(a[:, order]).astype(int), axis=1) >= 0)


def test_level_doubles_round_to_the_level_floats():
    rng = np.random.default_rng(5)
    nx, ny, nt, nz = 9, 4, 2, 6
    ps = rng.uniform(600, 1040, (nt, ny, nx)).astype(np.float32)
    c = rng.uniform(0, 1, nz)
    for lv in (vr.Levels(vr.AXIS, nz, axis=1000 * c), vr.Levels(vr.SIGMA, nz, sigma=c, ptop=5.0, ps=ps),
               vr.Levels(vr.HYBRID_SIGMA, nz, a=0.3 * c, b=c * c, p0=1000.0, ps=ps), vr.Levels(vr.HYBRID_SIGMA_AP, nz, ap=300 * c, b=c * c, ps=ps),
               vr.Levels(vr.FIELD, nz, field=rng.uniform(1, 1000, (nt, nz, ny, nx)))):
        d = vl.level_field_double(lv, nt, ny, nx)
        assert d.dtype == np.float64 and np.array_equal(d.astype(np.float32), vr.level_field(lv, nt, ny, nx))


def test_ocean_depth_field():
    rng = np.random.default_rng(6)
    nx, ny, nt, nz = 6, 5, 3, 4
    s, C = -rng.uniform(0, 1, nz), -rng.uniform(0, 1, nz)
    depth, eta = rng.uniform(5, 4000, (ny, nx)), rng.uniform(-1, 1, (nt, ny, nx))
    for gen, fn in ((1, vl.ocean_s_g1_z), (2, vl.ocean_s_g2_z)):
        got = vl.ocean_depth_field(gen, s, C, 20.0, depth, eta, nt)
        none = vl.ocean_depth_field(gen, s, C, 20.0, depth, None, nt)
        assert got.shape == none.shape == (nt, nz, ny, nx) and got.dtype == np.float32
        for t, k, j, i in ((0, 0, 0, 0), (2, 3, 4, 5), (1, 2, 3, 1)):
            assert got[t, k, j, i] == np.float32(-fn(depth[j, i], 20.0, eta[t, j, i], s[k], C[k]))
            assert none[t, k, j, i] == np.float32(-fn(depth[j, i], 20.0, 0.0, s[k], C[k]))
