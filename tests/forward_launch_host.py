"""fimex_amd/csrc/forward_launch.hpp on the CPU: tests/forward_launch_host.cc compiled with g++ into a temporary directory and called
through ctypes (the way tests/staged_layout_host.py wraps staged_layout.hpp).  The GPU tests of the forward slice loops ask the same
function, with the figures of plan.info(), which kernel a call takes and how it cuts the batch."""
import collections
import ctypes
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED, LANE, WAVE, MEDIAN_WAVE, MEDIAN_AS_MAX = range(5)  # Family
FAMILY_NAMES = ["tiled", "lane", "wave", "median-wave", "median-as-max"]
MEDIAN = 2  # Aggregate::Median; a forward method's aggregate is (method - FWD_SUM) % 5
# Tuning's members in order, and the switch of the tuning build each one carries (FIMEX_AMD_<NAME>)
KNOBS = ["FWD_TILED", "FWD_ZPB", "FWD_WAVE", "FWD_MEDIAN_SHORT", "FWD_MEDIAN_WAVE_MIN", "FWD_MEDIAN_WAVE", "FWD_MEDIAN_ZC"]
_lib = None

Launch = collections.namedtuple("Launch", "family zc ahead rank rankAll zPerBlock chunks laneGridX chunksFit meanBucket")


def load():
    global _lib
    if _lib is not None:
        return _lib
    d = tempfile.mkdtemp(prefix="forward_launch_")
    so = os.path.join(d, "libforward_launch_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "fimex_amd", "csrc"),
                    os.path.join(ROOT, "tests", "forward_launch_host.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.fl_forward_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fl_forward_launch.restype = None
    _lib = lib
    return lib


def forward_launch(nOut, nz, mappedSourceCells, undefinedCells, maxBucket, aggregate, tilesValid, knobs=None):
    """forward_launch() of forward_launch.hpp; knobs: {switch name: value} of the tuning build, none on the product build"""
    knobs = dict(knobs or {})
    tuning = (ctypes.c_int * len(KNOBS))(*[int(knobs.pop(k, -1)) for k in KNOBS])
    assert not knobs, "not a switch of the forward launcher: %s" % sorted(knobs)
    args = (ctypes.c_uint64 * 6)(nOut, nz, mappedSourceCells, undefinedCells, maxBucket, aggregate)
    out = (ctypes.c_uint64 * 9)()
    mean = ctypes.c_double(0.0)
    load().fl_forward_launch(args, 1 if tilesValid else 0, tuning, out, ctypes.byref(mean))
    v = [int(x) for x in out]
    return Launch(v[0], v[1], v[2], bool(v[3]), bool(v[4]), v[5], v[6], v[7], bool(v[8]), mean.value)


def launch_of_plan(info, nz, knobs=None):
    """the launch of a forward plan with these plan.info() figures; a plan holds a tiled form where it reports staged cells"""
    aggregate = (info["funcType"] - 5) % 5
    return forward_launch(info["outX"] * info["outY"], nz, info["mappedSourceCells"], info["undefinedCells"], info["maxBucket"], aggregate,
                          info["stagedCells"] > 0, knobs)


def chunk_lengths(launch, nz):
    """slices of every z chunk (z0 = chunk * zPerBlock, z1 = min(nz, z0 + zPerBlock))"""
    return [min(nz, (c + 1) * launch.zPerBlock) - c * launch.zPerBlock for c in range(launch.chunks)]


def chunk_passes(launch, nz):
    """per z chunk: (full passes of the lane kernel's ZC-slice loop, slices of the short last pass behind them)"""
    return [(n // launch.zc, n % launch.zc) for n in chunk_lengths(launch, nz)]
