"""Extraction on the GPU: fimex_amd_extract_apply_* byte for byte against tests/extract_ref.pick on every path of the
kernel -- every element size, every load width, head and tail, single-run and multi-run rows, merged and folded dimensions, eight
dimensions, the grid-stride loop, offsets beyond 2^32 -- and fimex_amd_extract_bounding_box_host against the stored fields of
coordTest.nc.  The output always lies between 32 guard bytes of 0xAB that must survive."""
import numpy as np
import pytest

import derived_ref as dr
import extract_ref as ref
from extract_ref import BOXES, coordtest

pytestmark = pytest.mark.gpu

GUARD = 32
STERE = "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +units=m +a=6.371e+06 +e=0 +no_defs"  # projection_1 of coordTest.nc
LONLAT = "+proj=latlong +R=6.371e6"
CROP = [(37, None, 3, 33), (7, None, 1, 5), (5, None, 0, 5)]  # [5][7][37]: x 3..35, y 1..5, all z


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def source(dims, dtype, seed=0):
    """Random bytes in the shape of the source, so that floats hold NaNs with payloads too."""
    n = int(np.prod([d[0] for d in dims]))
    raw = np.random.default_rng(seed).integers(0, 256, n * np.dtype(dtype).itemsize, dtype=np.uint8)
    return raw.view(dtype).reshape([d[0] for d in dims][::-1])


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def apply_device(fa, plan, src, inShift=0, outShift=0):
    """The device entry with source and output `inShift` / `outShift` elements behind a 16-byte boundary; returns the output bytes
    after checking the guards."""
    import torch
    elem, outBytes = src.dtype.itemsize, plan.info.outElements * src.dtype.itemsize
    d_in = torch.zeros(src.nbytes + 16 + inShift * elem, dtype=torch.uint8, device="cuda")
    d_in[inShift * elem:inShift * elem + src.nbytes] = torch.from_numpy(as_bytes(src).copy()).cuda()
    d_out = torch.full((2 * GUARD + outBytes + 16 + outShift * elem,), 0xAB, dtype=torch.uint8, device="cuda")
    first = GUARD + outShift * elem
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    plan.apply_device(d_in.data_ptr() + inShift * elem, fa.cdm_type_of(src.dtype), d_out.data_ptr() + first, stream=_stream())
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert np.all(raw[:first] == 0xAB) and np.all(raw[first + outBytes:] == 0xAB), "wrote outside the output"
    return raw[first:first + outBytes]


def check(fa, dims, dtype=np.int16, seed=0, shifts=((0, 0),), plan=None):
    src = source(dims, dtype, seed)
    want = as_bytes(ref.pick(src, dims))
    plan = plan or fa.ExtractPlan(dims)
    assert plan.info.outElements * src.dtype.itemsize == want.size
    for inShift, outShift in shifts:
        got = apply_device(fa, plan, src, inShift, outShift)
        assert np.array_equal(got, want), (dims, np.dtype(dtype).name, inShift, outShift, int((got != want).sum()))
    return plan


@pytest.mark.parametrize("cdmType", sorted(dr.DTYPES), ids=lambda t: np.dtype(dr.DTYPES[t]).name)
def test_every_type_and_alignment(fa, cdmType):
    """Source and destination 0, 1 and 3 elements behind a 16-byte boundary, independently: every load width from the element size to
    16 bytes occurs, and head and tail are not empty.  Rows of 1, 3, 16 / elem and 16 / elem + 1 columns as well as 33."""
    dtype = np.dtype(dr.DTYPES[cdmType])
    shifts = [(i, o) for i in (0, 1, 3) for o in (0, 1, 3)]
    check(fa, CROP, dtype, seed=cdmType, shifts=shifts)
    per = 16 // dtype.itemsize
    for outX in (1, 3, per, per + 1):
        check(fa, [(37, None, 3, outX)] + CROP[1:], dtype, seed=cdmType + outX, shifts=[(0, 0), (1, 3), (3, 1)])


RUNS = np.array([0, 1, 3, 6, 7, 8] + list(range(20, 37)))


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_rows_of_several_runs(fa, dtype):
    shifts = [(0, 0), (1, 3)]
    # a window that starts inside the run 6, 7, 8 and ends inside the run 20..36
    check(fa, [(37, RUNS, 4, 12), (7, None, 1, 5), (5, None, 0, 5)], dtype, 1, shifts)
    check(fa, [(37, RUNS), (7, None), (5, None)], dtype, 2, shifts)
    # every second x and every third y
    check(fa, [(37, np.arange(0, 37, 2)), (7, np.arange(0, 7, 3)), (5, None)], dtype, 3, shifts)
    # single columns only: one of them, and three that are no neighbours
    check(fa, [(37, [5]), (7, None), (5, None)], dtype, 4, shifts)
    check(fa, [(37, [5, 9, 30]), (7, None), (5, None)], dtype, 5, shifts)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_the_multi_run_path_on_single_run_rows(fa, monkeypatch, tuning_build, dtype):
    """FIMEX_AMD_EXTRACT_GENERAL=1 sends a crop through the run table: the same bytes as the default path."""
    src = source(CROP, dtype, 6)
    plan = fa.ExtractPlan(CROP)
    assert plan.info.fastestRuns == 1
    default = apply_device(fa, plan, src, 1, 3)
    monkeypatch.setenv("FIMEX_AMD_EXTRACT_GENERAL", "1")
    forced = apply_device(fa, plan, src, 1, 3)
    assert np.array_equal(forced, default) and np.array_equal(default, as_bytes(ref.pick(src, CROP)))


def test_merged_and_folded_dimensions(fa):
    shifts = [(0, 0), (3, 1)]
    # levels over whole planes: one dimension of three runs
    levels = [(40, None), (8, None), (6, None), (9, [0, 2, 3, 8])]
    plan = check(fa, levels, np.int16, 1, shifts)
    assert (plan.info.kernelDims, plan.info.fastestRuns) == (1, 3)
    # a time window (2, 3) on a picked time list, levels picked as well
    times = [(40, None), (8, None), (6, [1, 2, 5]), (9, [0, 2, 3, 5, 8], 2, 3)]
    check(fa, times, np.float32, 2, shifts)
    # a dimension of length 1 in the middle, whole, and one of length 3 cut to one position
    assert check(fa, [(40, None), (1, None), (8, None), (9, [0, 2, 3, 8])], np.int16, 3, shifts).info.kernelDims == 1
    assert check(fa, [(40, None), (3, None, 1, 1), (8, None), (9, [0, 2, 3, 8])], np.int16, 4, shifts).info.kernelDims == 2
    # one element
    check(fa, [(40, None, 7, 1), (8, [2, 6], 1, 1)], np.float64, 5, shifts)
    # D9: the reference would emit these run-major; the row-major array is the expectation
    for dims in ([(37, RUNS), (7, None), (5, None)], [(40, None, 2, 30), (8, [1, 2, 6]), (6, None, 1, 4), (9, [3, 4])]):
        plan = check(fa, dims, np.int16, 6, shifts)
        assert plan.info.referenceOrderDiffers == 1 and ref.order_differs(dims)
        src = source(dims, np.int16, 6)
        assert not np.array_equal(ref.reference_join(src, dims), ref.pick(src, dims).ravel())


@pytest.mark.parametrize("seed", range(20))
def test_eight_dimensions(fa, seed):
    rng = np.random.default_rng(100 + seed)
    dims = []
    for length in (5, 2, 3, 2, 2, 3, 2, 2):
        positions = None
        if rng.random() < 0.6:
            positions = np.sort(rng.choice(length, int(rng.integers(1, length + 1)), replace=False))
        limit = length if positions is None else len(positions)
        start = int(rng.integers(0, limit))
        dims.append((length, positions, start, int(rng.integers(1, limit - start + 1))))
    dtype = (np.uint8, np.int16, np.float32, np.float64)[seed % 4]
    check(fa, dims, dtype, seed, [(0, 0), (1, 1)])


BIG_CROP = [(300, None, 7, 281), (70, None, 3, 60), (4, None)]  # 67 440 elements: 33 workgroups of 16-byte groups of shorts


def test_the_grid_stride_loop(fa, monkeypatch, tuning_build):
    """With the grid capped at two workgroups every lane strides several times."""
    monkeypatch.setenv("FIMEX_AMD_EXTRACT_MAX_BLOCKS", "2")
    for dtype in (np.int16, np.float64):
        check(fa, BIG_CROP, dtype, 7, [(0, 0), (1, 3)])
    check(fa, [(300, np.arange(1, 300, 2)), (70, None, 3, 60), (4, None)], np.int16, 8, [(1, 3)])


def test_more_than_one_workgroup(fa):
    for dtype in (np.int16, np.float64):
        check(fa, BIG_CROP, dtype, 7, [(0, 0), (1, 3)])
    check(fa, [(300, np.arange(1, 300, 2)), (70, None, 3, 60), (4, None)], np.int16, 8, [(1, 3)])


def test_source_offsets_beyond_32_bits(fa):
    """A uint8 source of 65 538 rows of 65 536 bytes: the second picked row starts 4 294 901 760 + 65 472 bytes in."""
    import torch
    nx, ny = 65536, 65538
    if torch.cuda.mem_get_info()[0] < 6 * 2 ** 30:
        pytest.skip("less than 6 GiB of device memory free")
    dims = [(nx, None, 65472, 64), (ny, [0, ny - 1])]
    plan = fa.ExtractPlan(dims)
    assert plan.info.inElements == nx * ny == 4295098368
    d_in = torch.empty(nx * ny, dtype=torch.uint8, device="cuda")
    rows = np.random.default_rng(9).integers(0, 256, (2, 64), dtype=np.uint8)
    for k, y in enumerate((0, ny - 1)):
        assert y * nx + 65472 + 64 <= nx * ny
        d_in[y * nx + 65472:y * nx + 65472 + 64] = torch.from_numpy(rows[k]).cuda()
    assert (ny - 1) * nx + 65472 > 2 ** 32
    d_out = torch.full((2 * GUARD + 128,), 0xAB, dtype=torch.uint8, device="cuda")
    plan.apply_device(d_in.data_ptr(), fa.CDM_UCHAR, d_out.data_ptr() + GUARD, stream=_stream())
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    del d_in
    assert np.all(raw[:GUARD] == 0xAB) and np.all(raw[GUARD + 128:] == 0xAB)
    assert np.array_equal(raw[GUARD:GUARD + 128], rows.reshape(-1))


def test_empty_results(fa):
    """An empty list and a window of size 0: OK with NULL pointers, and an output that is given stays untouched."""
    import torch
    d_out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_in = torch.zeros(37 * 7 * 2, dtype=torch.uint8, device="cuda")
    for dims in ([(37, None), (7, [])], [(37, None, 5, 0), (7, [1, 2])], [(37, None), (7, [1, 2], 2, 0)]):
        plan = fa.ExtractPlan(dims)
        assert (plan.info.outElements, plan.info.inElements, plan.info.kernelDims) == (0, 37 * 7, 0)
        plan.apply_device(None, fa.CDM_SHORT, None, stream=_stream())
        plan.apply_device(d_in.data_ptr(), fa.CDM_SHORT, d_out.data_ptr(), stream=_stream())
        assert plan.apply_host(np.zeros((7, 37), np.int16)).size == 0
        with pytest.raises(fa.FimexAmdError, match="data type 6"):
            plan.apply_device(None, 6, None)  # the type is checked even then
    torch.cuda.synchronize()
    assert bool((d_out == 0xAB).all())


def test_apply_refusals(fa):
    """What needs a plan to be refused: the type, NULL and misaligned buffers, any overlap of output and input."""
    import torch
    plan = fa.ExtractPlan(CROP)  # reads 1295 shorts, writes 825
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    P = buf.data_ptr()
    inBytes, outBytes = 1295 * 2, 825 * 2
    for bad, match in ((0, "data type 0"), (6, "data type 6")):  # NAT and STRING
        with pytest.raises(fa.FimexAmdError, match=match):
            plan.apply_device(P, bad, P + 4096)
    for args in ((None, P), (P, None)):
        with pytest.raises(fa.FimexAmdError, match="NULL data buffer"):
            plan.apply_device(args[0], fa.CDM_SHORT, args[1])
    for args in ((P + 1, P + 4096), (P, P + 4097)):
        with pytest.raises(fa.FimexAmdError, match="not aligned to its element size"):
            plan.apply_device(args[0], fa.CDM_SHORT, args[1])
    for d_out in (P, P + inBytes - 2, P - outBytes + 2, P + 1000):
        with pytest.raises(fa.FimexAmdError, match="overlaps the input buffer"):
            plan.apply_device(P, fa.CDM_SHORT, d_out)
    host = np.zeros(1295 + 825, np.int16)
    lib = fa.load()
    assert lib.fimex_amd_extract_apply_host(plan._h, host.ctypes.data, fa.CDM_SHORT, host.ctypes.data + 2000) == fa.ERROR
    assert "overlaps the input buffer" in lib.fimex_amd_last_error().decode()
    plan.apply_device(P, fa.CDM_SHORT, P + inBytes)  # touching is no overlap
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        plan.apply_host(np.zeros(7, np.int16))


def test_host_form_equals_device_form(fa):
    for dims, dtype in ((CROP, np.float32), ([(37, RUNS, 4, 12), (7, np.arange(0, 7, 3)), (5, None)], np.int16)):
        src = source(dims, dtype, 11)
        plan = fa.ExtractPlan(dims)
        got = plan.apply_host(src)
        assert got.shape == ref.pick(src, dims).shape and got.dtype == src.dtype
        assert np.array_equal(as_bytes(got), apply_device(fa, plan, src)) and np.array_equal(as_bytes(got), as_bytes(ref.pick(src, dims)))
        assert np.array_equal(as_bytes(src), as_bytes(source(dims, dtype, 11)))  # the input is left as it was


@pytest.mark.parametrize("box,xs,ys", BOXES, ids=["inside", "across180", "empty"])
def test_bounding_box_on_coordtest(fa, box, xs, ys):
    c = coordtest()
    assert c["proj"] == STERE
    gx, gy = fa.extract_bounding_box_host(STERE, LONLAT, c["x"], c["y"], *box)
    assert gx.tolist() == xs and gy.tolist() == ys
    assert gx.dtype == np.uintp


def test_bounding_box_on_a_degree_grid_across_the_date_line(fa):
    x, y = -180.0 + 0.5 * np.arange(720), 40.0 + 0.5 * np.arange(61)
    south, north, west, east = 50.1, 60.1, 170.2, -170.3
    for axis, bounds in ((x, (west, east)), (y, (south, north))):
        assert min(np.abs(axis - b).min() for b in bounds) > 1e-6
    wantX = np.flatnonzero(~((x > east) & (x < west)))  # src/CDMExtractor.cc:503
    wantY = np.flatnonzero((y >= south) & (y <= north))
    assert np.flatnonzero(np.diff(wantX) > 1).size == 1 and wantX[0] == 0 and wantX[-1] == 719  # two runs
    gx, gy = fa.extract_bounding_box_host(LONLAT, LONLAT, x, y, south, north, west, east, axesInDegree=True)
    assert np.array_equal(gx, wantX) and np.array_equal(gy, wantY)
    # the same box the other way round keeps the complement in x
    gx, gy = fa.extract_bounding_box_host(LONLAT, LONLAT, x, y, south, north, east, west, axesInDegree=True)
    assert np.array_equal(gx, np.flatnonzero((x >= east) & (x <= west))) and np.array_equal(gy, wantY)
    # more columns than a wave and a box in one corner
    gx, gy = fa.extract_bounding_box_host(LONLAT, LONLAT, x, y, 69.9, 70.1, 179.4, 179.6, axesInDegree=True)
    assert gx.tolist() == [719] and gy.tolist() == [60]


def test_bounding_box_leaves_failed_points_out(fa):
    """Divergence D10.  Beyond the disk of the orthographic projection the inverse fails; across 180 degrees a literal restatement of
    src/CDMExtractor.cc:501-506 would keep such a point (no comparison with NaN is true)."""
    ortho = "+proj=ortho +lat_0=90 +lon_0=0 +R=6.371e6"
    x, y = np.array([-7e6, 1e6, 3e6]), np.array([1e6, 3e6])
    lon, lat = fa.project_axes_host(ortho, LONLAT, x, y)
    assert not np.isfinite(lon[:, 0]).any() and np.isfinite(lon[:, 1:]).all()
    box = (0.0, 90.0, 10.0, -10.0)
    wantX, wantY = ref.bounding_box(np.degrees(lon), np.degrees(lat), *box)
    assert wantX.tolist() == [1, 2] and wantY.tolist() == [0, 1]
    gx, gy = fa.extract_bounding_box_host(ortho, LONLAT, x, y, *box)
    assert gx.tolist() == [1, 2] and gy.tolist() == [0, 1]


def test_chain_from_box_to_scaled_values(fa):
    """Bounding box -> two fimex_amd_extract_dim -> plan -> apply on air_temperature of coordTest.nc in its stored type -> scaled
    read: the numpy crop of the variable, scaled by derived_ref."""
    import torch
    c = coordtest()
    var = c["air_temperature"]  # [4][11][11] short
    gx, gy = fa.extract_bounding_box_host(STERE, LONLAT, c["x"], c["y"], *BOXES[0][0])
    dims = [(11, gx), (11, gy), (4, None)]
    plan = fa.ExtractPlan(dims)
    n = plan.info.outElements
    assert n == 4 * 6 * 7
    d_in = torch.from_numpy(as_bytes(var).copy()).cuda()
    d_raw = torch.zeros(n * 2, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
    plan.apply_device(d_in.data_ptr(), fa.CDM_SHORT, d_raw.data_ptr(), stream=_stream())
    fill, scale = c["air_temperature_fill"], c["air_temperature_scale"]
    fa.convert_scaled_device(d_raw.data_ptr(), fa.CDM_SHORT, n, fill, scale, 0.0, fa.CDM_FLOAT, float("nan"), 1.0, 0.0, d_out.data_ptr(),
                             stream=_stream())
    torch.cuda.synchronize()
    crop = np.ascontiguousarray(var[:, 2:8, 2:9])
    assert np.array_equal(d_raw.cpu().numpy().view(var.dtype), crop.reshape(-1))
    want = dr.convert_scaled(crop.reshape(-1), fill, scale, 0.0, dr.CDM_FLOAT, float("nan"), 1.0, 0.0)
    got = d_out.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert np.isfinite(got).sum() > n // 2
