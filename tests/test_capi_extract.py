"""The (8f n11) entries at the C boundary: both libraries export the eight symbols, the binding mirrors the header, the two CPU-only
entries agree with tests/extract_ref.py, and what can be refused without a device is refused with a message.  CPU only: nothing is
computed on a device.  (The refusals of an apply that need a plan, the overlap among them, are in tests/test_gpu_extract.py: a plan
cannot be made without a device.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import extract_ref as ref
from extract_ref import coordtest, random_reduction
from fimex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fimex_amd_extract_describe", "fimex_amd_extract_plan_create", "fimex_amd_extract_plan_destroy", "fimex_amd_extract_plan_info",
         "fimex_amd_extract_apply_device", "fimex_amd_extract_apply_host", "fimex_amd_extract_axis_range",
         "fimex_amd_extract_bounding_box_host")
NAN = float("nan")
STERE = "+proj=stere +lat_0=90 +lon_0=0 +lat_ts=60 +units=m +a=6.371e+06 +e=0 +no_defs"
LONLAT = "+proj=latlong +R=6.371e6"


HOST_HEADER = "fimex_amd_extract_host.h"


def _header(name="fimex_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared(text):
    return set(re.findall(r"\b(fimex_amd_[a-z0-9_]+)\s*\(", text))


def test_both_libraries_export_the_eight_symbols():
    for path in (capi.LIB_PATH, capi.TUNING_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(lib, name), "missing export in %s: %s" % (os.path.basename(path), name)


def test_header_and_binding_agree():
    """The six entries on device pointers or the CPU are in fimex_amd.h and capi.SYMBOLS; the two on host buffers have a header and a
    table of their own, as the host forms of n9 and n10 have (tests/test_gpu_host_entries.py lists the *_host entries of SYMBOLS)."""
    text, host = _header(), _header(HOST_HEADER)
    hostNames = sorted(n for n in NAMES if n.endswith("_host"))
    assert sorted(_declared(host)) == hostNames == sorted(capi.EXTRACT_HOST_SYMBOLS)
    assert sorted(n for n in _declared(text) if n.startswith("fimex_amd_extract_")) == sorted(set(NAMES) - set(hostNames))
    assert set(NAMES) - set(hostNames) <= set(capi.SYMBOLS) and not set(hostNames) & set(capi.SYMBOLS)
    assert int(re.search(r"#define FIMEX_AMD_EXTRACT_MAX_DIMS (\d+)", text).group(1)) == capi.EXTRACT_MAX_DIMS == 8
    for struct, binding in (("fimex_amd_extract_dim", capi.ExtractDim), ("fimex_amd_extract_info", capi.ExtractInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert fields == [name for name, _ in binding._fields_]
    # the number of arguments of every entry
    for name in NAMES:
        table = capi.EXTRACT_HOST_SYMBOLS if name in hostNames else capi.SYMBOLS
        args = re.search(r"\b%s\s*\((.*?)\)" % name, host if name in hostNames else text, flags=re.S).group(1)
        assert len(args.split(",")) == len(table[name][1]), name


def test_host_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "%s"\nint main(void){return FIMEX_AMD_EXTRACT_MAX_DIMS == 8 ? 0 : 1;}\n' % HOST_HEADER)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_describe_agrees_with_the_restatement():
    rng = np.random.default_rng(7)
    differing = 0
    for _ in range(1500):
        dims = random_reduction(rng, empty=0.05)
        info = capi.extract_describe(dims)
        assert info.inElements == int(np.prod([d[0] for d in dims]))
        assert info.outElements == int(np.prod([d[3] for d in dims]))
        assert bool(info.referenceOrderDiffers) == ref.order_differs(dims), dims
        differing += info.referenceOrderDiffers
        if info.outElements == 0:
            assert info.kernelDims == 0 and info.fastestRuns == 0
        else:
            assert 1 <= info.kernelDims <= sum(d[3] > 1 for d in dims) or info.kernelDims == 1
            assert 1 <= info.fastestRuns <= info.outElements
    assert differing >= 5


def test_describe_merges_and_counts_runs():
    # a crop of [5][7][37]: x 3..35 is one run but not whole, y 1..5 neither, z whole but the slowest: nothing merges
    crop = capi.extract_describe([(37, None, 3, 33), (7, None, 1, 5), (5, None, 0, 5)])
    assert (crop.inElements, crop.outElements, crop.kernelDims, crop.fastestRuns, crop.referenceOrderDiffers) == (5 * 7 * 37, 5 * 5 * 33, 3, 1, 0)
    # levels {0, 2, 3, 8} of [9][6][8][40] over whole planes: x, y and the third dimension merge into the level dimension, whose
    # neighbours 2, 3 join: one dimension of three runs
    levels = capi.extract_describe([(40, None), (8, None), (6, None), (9, [0, 2, 3, 8])])
    assert (levels.outElements, levels.kernelDims, levels.fastestRuns, levels.referenceOrderDiffers) == (4 * 6 * 8 * 40, 1, 3, 0)
    # every second column: as many runs as columns; y whole but x is not, so nothing merges; y is not reduced and slower: D9
    second = capi.extract_describe([(37, np.arange(0, 37, 2)), (7, None), (5, None, 2, 1)])
    assert (second.outElements, second.kernelDims, second.fastestRuns, second.referenceOrderDiffers) == (19 * 7, 2, 19, 1)
    # a picked single column: the fastest dimension left has stride 37, every position is a run of its own
    column = capi.extract_describe([(37, [5]), (7, None), (5, None)])
    assert (column.outElements, column.kernelDims, column.fastestRuns) == (35, 1, 35)
    # one element: everything folds into the base offset
    one = capi.extract_describe([(37, None, 4, 1), (7, [2, 6], 1, 1)])
    assert (one.outElements, one.kernelDims, one.fastestRuns) == (1, 1, 1)
    # a dimension of length 1 between two whole ones does not stop the merge; one of size 1 and length 3 does
    assert capi.extract_describe([(8, None), (1, None), (6, None), (4, [1, 3])]).kernelDims == 1
    assert capi.extract_describe([(8, None), (3, None, 1, 1), (6, None), (4, [1, 3])]).kernelDims == 2


def test_axis_range_agrees_with_the_restatement():
    sigma = coordtest()["sigma"]
    assert capi.extract_axis_range(sigma, 0.5, 0.85) == (1, 2)  # test/testExtractor.cc:163-166
    assert capi.extract_axis_range(sigma, -0.1, -0.05)[1] == 0  # :168-172
    cases = [(sigma, 0.5, 0.85), (sigma, -0.1, -0.05), (sigma[::-1], 0.5, 0.85), (sigma[::-1], 0.85, 1.0), (sigma[::-1], 0.2, 0.3),
             ([], 0.0, 1.0), ([4.0], 4.0, 4.0), ([4.0], 4.1, 5.0), ([4.0], 5.0, 3.0), ([1.0, 1.0, 2.0], 1.0 + 0.5e-5, 2.0 - 0.5e-5),
             ([1.0, 1.0, 2.0], 1.0 + 2e-5, 2.0 - 2e-5), ([0.0, 100.0, 200.0, 300.0], 101.0, 199.0), ([0.0, 100.0, 200.0, 300.0], 101.5, 198.5),
             ([300.0, 200.0, 100.0, 0.0], 101.0, 199.0)]
    rng = np.random.default_rng(3)
    for _ in range(300):
        axis = np.cumsum(rng.integers(0, 3, int(rng.integers(1, 9)))) * 0.5  # ascending with ties
        if rng.random() < 0.5:
            axis = axis[::-1]
        a, b = np.sort(rng.choice(np.arange(-1.0, 9.0, 0.25), 2))
        cases.append((axis, a + rng.choice([0.0, 1e-5, -1e-5, 0.005]), b))
    for axis, a, b in cases:
        assert capi.extract_axis_range(axis, a, b) == ref.axis_range(axis, a, b), (axis, a, b)


def _refused(call, *args, match):
    with pytest.raises(capi.FimexAmdError, match=match):
        call(*args)


BAD_REDUCTIONS = [
    ([], "nDims == 0"),
    ([(2, None)] * 9, "more than 8 dimensions"),
    ([(4, None), (0, None, 0, 1)], "dimension 1 has length 0 and a window of size 1"),
    ([(4, [0, 2, 2])], "dimension 0 are not strictly ascending at entry 2"),
    ([(4, None), (4, [3, 1])], "dimension 1 are not strictly ascending at entry 1"),
    ([(4, [0, 4])], "position 4 of dimension 0 is beyond its length 4"),
    ([(4, None, 2, 3)], r"window \(2, 3\) of dimension 0 is beyond its reduced length 4"),
    ([(4, None), (9, [1, 5, 7], 2, 2)], r"window \(2, 2\) of dimension 1 is beyond its reduced length 3"),
    ([(4, None, 5, 0)], r"window \(5, 0\) of dimension 0 is beyond its reduced length 4"),
    ([(4, None, 1, 2 ** 64 - 1)], "beyond its reduced length"),  # start + size wraps
    ([(2 ** 33, None, 0, 1)] * 2, "more elements than size_t counts"),
]


@pytest.mark.parametrize("dims,match", BAD_REDUCTIONS, ids=[m[:24] for _, m in BAD_REDUCTIONS])
def test_bad_reductions_are_refused_without_a_device(dims, match):
    _refused(capi.extract_describe, dims, match=match)
    _refused(capi.ExtractPlan, dims, match=match)


def test_null_arguments_are_refused_without_a_device():
    lib = capi.load()
    info, plan = capi.ExtractInfo(), ctypes.c_void_p()
    dim = (capi.ExtractDim * 1)()
    dim[0].length, dim[0].reduced, dim[0].nPositions, dim[0].size = 4, 1, 2, 2  # positions stay NULL

    def refused(rc, match):
        assert rc == capi.ERROR and re.search(match, lib.fimex_amd_last_error().decode())

    refused(lib.fimex_amd_extract_describe(None, 1, ctypes.byref(info)), "NULL dimensions")
    refused(lib.fimex_amd_extract_describe(dim, 1, None), "NULL argument")
    refused(lib.fimex_amd_extract_describe(dim, 1, ctypes.byref(info)), "NULL positions of dimension 0")
    refused(lib.fimex_amd_extract_plan_create(dim, 1, ctypes.byref(plan)), "NULL positions of dimension 0")
    refused(lib.fimex_amd_extract_plan_create(dim, 1, None), "NULL argument")
    refused(lib.fimex_amd_extract_plan_info(None, ctypes.byref(info)), "NULL argument")
    # 1 is no pointer: the plan is looked at first, on the device form and the host form alike
    refused(lib.fimex_amd_extract_apply_device(None, 1, capi.CDM_SHORT, 1, None), "NULL extract plan")
    refused(lib.fimex_amd_extract_apply_host(None, 1, capi.CDM_SHORT, 1), "NULL extract plan")
    assert lib.fimex_amd_extract_plan_destroy(None) == capi.OK
    dim[0].nPositions = dim[0].size = 0  # an empty list needs no array
    assert lib.fimex_amd_extract_describe(dim, 1, ctypes.byref(info)) == capi.OK and info.outElements == 0 and info.inElements == 4


def test_bad_axis_ranges_are_refused():
    _refused(capi.extract_axis_range, [0.0, NAN, 2.0], 0.0, 1.0, match="the axis is NaN at position 1")
    _refused(capi.extract_axis_range, [0.0, 1.0], NAN, 1.0, match="bound of the range is NaN")
    _refused(capi.extract_axis_range, [0.0, 1.0], 0.0, NAN, match="bound of the range is NaN")
    lib = capi.load()
    start, size = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.fimex_amd_extract_axis_range(None, 3, 0.0, 1.0, ctypes.byref(start), ctypes.byref(size)) == capi.ERROR
    assert lib.fimex_amd_extract_axis_range(None, 0, 0.0, 1.0, None, ctypes.byref(size)) == capi.ERROR
    assert lib.fimex_amd_extract_axis_range(None, 0, 0.0, 1.0, ctypes.byref(start), ctypes.byref(size)) == capi.OK


@pytest.mark.parametrize("box,match", [
    ((50.0, 40.0, 0.0, 10.0), "south > north: 50>40"),
    ((-90.5, 40.0, 0.0, 10.0), "south outside domain: -90.5"),
    ((40.0, 91.0, 0.0, 10.0), "north outside domain: 91"),
    ((40.0, 50.0, -180.5, 10.0), "west outside domain: -180.5"),
    ((40.0, 50.0, 0.0, 181.0), "east outside domain: 181"),
])
def test_bad_boxes_are_refused_without_a_device(box, match):
    """src/CDMExtractor.cc:442-447, before the axes or a device are looked at."""
    _refused(capi.extract_bounding_box_host, STERE, LONLAT, [0.0, 1.0], [0.0, 1.0], *box, match="reduceLatLonBoundingBox " + match)
    lib = capi.load()
    n = ctypes.c_size_t()
    assert lib.fimex_amd_extract_bounding_box_host(None, None, None, 5, None, 5, 0, *box, None, ctypes.byref(n), None, ctypes.byref(n)) == capi.ERROR
    assert re.search(match, lib.fimex_amd_last_error().decode())


def test_empty_axes_give_empty_lists_without_a_device():
    gx, gy = capi.extract_bounding_box_host(STERE, LONLAT, [], [0.0, 1.0], 40.0, 50.0, 0.0, 10.0)
    assert gx.size == 0 and gy.size == 0


def test_without_a_device_the_compute_entries_fail_loudly():
    """No CPU fallback: a plan and a bounding box need a gfx950 device; with one, the same calls succeed."""
    dims = [(37, None, 3, 33), (7, None, 1, 5)]
    if capi.device_count() > 0:
        assert capi.ExtractPlan(dims).info.outElements == 33 * 5
        return
    _refused(capi.ExtractPlan, dims, match="no HIP device|gfx950")
    _refused(capi.ExtractPlan, [(4, [])], match="no HIP device|gfx950")  # an empty result too: a plan lives on a device
    _refused(capi.extract_bounding_box_host, STERE, LONLAT, [0.0, 1.0], [0.0, 1.0], 40.0, 50.0, 0.0, 10.0, match="no HIP device|gfx950")
