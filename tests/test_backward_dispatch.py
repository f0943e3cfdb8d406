"""fimex_amd/csrc/backward_dispatch.hpp, the rule that names the kernel of every call of the backward regrid, on the CPU: compiled
with g++ (tests/backward_dispatch_host.cc) and compared, answer by answer, with the conditions the entry points carried before the
header existed (tests/backward_dispatch_ref.py) -- over every setting of the eight switches, every kind of plan, and calls on both
sides of every threshold.  A few million rows, one call into the library per table.  And the guard that keeps the rule in one
place: the eight switches are read by one function."""
import itertools
import os
import re

import numpy as np
import pytest

import backward_dispatch_host as host
import backward_dispatch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fimex_amd", "csrc")

SWITCH_VALUES = dict(STAGED=(0, 1), STAGED_NEAREST=(0, 1), STAGED2=(0, 1, 2), TYPED_FUSED=(0, 1, 2), TYPED_STAGED=(0, 1), TYPED_STAGED2=(0, 1),
                     VECTOR_FUSED=(0, 1), STAGED_MIN_NZ=(1, 4))
FUNC_TYPES = (ref.FUNC_NEAREST, ref.FUNC_COORD_NN, ref.FUNC_COORD_NN_KD, ref.FUNC_BILINEAR, ref.FUNC_BICUBIC)
# inX, inY, outX, outY.  320 x 18: slices of 1- and 2-byte elements are multiples of 4 bytes; 321 x 18: only those of 2-byte
# elements; 323 x 17: neither.  Then the gather kernel's descriptor (8 slices of 4-byte cells behind 2^32 - 1 bytes): the last
# grid inside it, the first one beyond it by its source, and one beyond it by its output.
GRIDS = ((320, 18, 256, 16), (321, 18, 256, 16), (323, 17, 256, 16), (134217727, 1, 256, 16), (16384, 8192, 256, 16), (320, 18, 16384, 8192))
NZ = (1, 3, 4, 5, 2 ** 32)
TYPES = tuple(range(12))  # every fimex_amd_datatype, NAT and STRING too
UNEQUAL_PAIRS = ((ref.CDM_SHORT, ref.CDM_USHORT), (ref.CDM_USHORT, ref.CDM_SHORT), (ref.CDM_SHORT, ref.CDM_INT), (ref.CDM_UCHAR, ref.CDM_CHAR),
                 (ref.CDM_FLOAT, ref.CDM_SHORT))


def _switch_table():
    return np.array(list(itertools.product(*(SWITCH_VALUES[k] for k in ref.SWITCH_COLUMNS))), np.int64)


def _plan_table():
    rows = [(ref.KIND_OF_FUNC[f], f, fast, first, second) + g
            for f in FUNC_TYPES for fast in (0, 1) for first in (0, 1) for second in (0, 1) for g in GRIDS]
    return np.array(rows, np.int64)


def _float_calls():
    return np.array([(nz, ref.CDM_FLOAT, ref.CDM_FLOAT, 1, shapes, chunks) for nz in NZ for shapes in (0, 1) for chunks in (0, 1)], np.int64)


def _typed_calls():
    pairs = [(t, t) for t in TYPES] + list(UNEQUAL_PAIRS)
    return np.array([(nz, t, t2, aligned, 0, 0) for nz in NZ for t, t2 in pairs for aligned in (0, 1)], np.int64)


def _columns(table, names, axis):
    """The columns of a table as arrays that broadcast to [switch][plan][call]."""
    shape = [1, 1, 1]
    shape[axis] = len(table)
    return {n: table[:, i].reshape(shape) for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def lib():
    return host.load()


@pytest.fixture(scope="module")
def tables():
    s, p = _switch_table(), _plan_table()
    assert len(s) == 2 * 2 * 3 * 3 * 2 * 2 * 2 * 2 and len(p) == 5 * 8 * len(GRIDS)
    return s, p, _columns(s, ref.SWITCH_COLUMNS, 0), _columns(p, ref.PLAN_COLUMNS, 1)


def _same(got, want, what):
    want = np.broadcast_to(want, got.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d rows differ, the first at [switch, plan, call] = %s: header %d, parent's conditions %d" % (
        what, len(bad), got.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_plan_build_tries_the_forms_the_parent_tried(lib, tables):
    s, p, sw, plan = tables
    got = host.plan_build(lib, s, p)
    _same(got[:, :, 0], ref.builds_first(sw, plan)[:, :, 0].astype(np.int8), "builds_first")
    _same(got[:, :, 1], ref.builds_second(sw, plan)[:, :, 0].astype(np.int8), "builds_second")


def test_float_slices_pairs_lists_and_tune_run_what_the_parent_ran(lib, tables):
    s, p, sw, plan = tables
    c = _float_calls()
    call = _columns(c, ref.CALL_COLUMNS, 2)
    got = host.float_answers(lib, s, p, c)
    assert got.shape[:3] == (len(s), len(p), len(c))
    want_apply = ref.float_apply(sw, plan, call)
    _same(got[..., 0], want_apply.astype(np.int8), "float_apply")
    # fimex_amd_regrid_plan_launch_order reports an order exactly for the launches of the second form
    _same((got[..., 0] == ref.SECOND).astype(np.int8), ref.launch_order_is_reported(sw, plan, call).astype(np.int8), "launch order >= 0")
    _same(got[..., 1], ref.tune_has_choice(sw, plan, call).astype(np.int8), "tune_has_choice")
    _same(got[..., 2], ref.float_list(sw, plan, call).astype(np.int8), "float_list")
    _same(got[..., 3], ref.vector_fused(sw, plan, call).astype(np.int8), "vector_fused")
    for answer in (ref.SECOND, ref.FIRST, ref.GATHER):  # the table reaches every answer
        assert (got[..., 0] == answer).any()


def test_stored_types_pairs_and_lists_try_what_the_parent_tried(lib, tables):
    s, p, sw, plan = tables
    c = _typed_calls()
    call = _columns(c, ref.CALL_COLUMNS, 2)
    got = host.typed_answers(lib, s, p, c)
    assert got.size // 6 == len(s) * len(p) * len(c) > 3_000_000
    one = dict(call, type2=call["type"])  # a variable or a list has one type
    want = ref.typed_candidates(sw, plan, one)
    for k in range(4):
        _same(got[..., k], want[..., k], "typed_apply, candidate %d" % k)
    _same(got[..., 4], ref.typed_list(sw, plan, one).astype(np.int8), "typed_list")
    _same(got[..., 5], ref.vector_typed_fused(sw, plan, call).astype(np.int8), "vector_typed_fused")
    for first in (ref.SECOND, ref.FIRST, ref.GATHER, ref.THREE_PASSES):  # every kernel leads some list
        assert (got[..., 0] == first).any()
    assert got[..., 4].any() and got[..., 5].any()


def test_the_switches_of_the_rule_are_read_by_one_function():
    """A hand copy of a condition has to name a switch: the eight names, as the string literals tuning() takes, stand in
    fimex_amd/csrc only inside dispatch_switches (backward_plan.hip), once each."""
    literal = re.compile(r'"(%s)"' % "|".join(ref.SWITCH_COLUMNS))
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            lines = f.read().split("\n")
        for i, line in enumerate(lines):
            for m in literal.finditer(line):
                found.setdefault(m.group(1), []).append((name, i))
    assert sorted(found) == sorted(ref.SWITCH_COLUMNS), found
    with open(os.path.join(CSRC, "backward_plan.hip"), encoding="utf-8") as f:
        lines = f.read().split("\n")
    begin = lines.index("dispatch::Switches dispatch_switches()")
    end = begin + lines[begin:].index("}")
    for switch, places in found.items():
        assert len(places) == 1 and places[0][0] == "backward_plan.hip" and begin < places[0][1] < end, (switch, places)
