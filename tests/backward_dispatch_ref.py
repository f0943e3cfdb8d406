"""Which kernel serves a call of the backward regrid, written out from the conditions the entry points carried themselves at commit
1081fbd, the last one before fimex_amd/csrc/backward_dispatch.hpp -- file by file, each function citing the lines of that commit
it restates.  It is NOT written from the header: tests/test_backward_dispatch.py holds the header to it over the whole cross
product of switches, plans and calls, and tests/test_gpu_backward_dispatch.py holds the library's reported paths to it.

Every function takes three dicts, `sw`, `plan` and `call`, of numbers or of numpy arrays that broadcast against each other, and
returns booleans (or small integers) of the broadcast shape.

  sw    STAGED, STAGED_NEAREST, STAGED2, TYPED_FUSED, TYPED_STAGED, TYPED_STAGED2, VECTOR_FUSED, STAGED_MIN_NZ
  plan  kind (NEAREST / BILINEAR / BICUBIC below), funcType, fast (FIMEX_AMD_BICUBIC_FAST), first, second (plan.staged.valid,
        plan.staged2.valid), inX, inY, outX, outY
  call  nz (a list: list_slices of it, slice_list.hpp), type, type2 (pairs: the v component), aligned (every source pointer is a
        multiple of 4), shapes (plan.staged2Alt.valid), chunks (chunk_xcd_chunk_count(nz, zpb) != 0) -- the last two for tune only

What the launchers find out only when they run stays outside, as it does in the header: whether staged2_typed_form could build
the stored type's form, and the list kernels' list_shape.
"""
import numpy as np

SWITCH_COLUMNS = ("STAGED", "STAGED_NEAREST", "STAGED2", "TYPED_FUSED", "TYPED_STAGED", "TYPED_STAGED2", "VECTOR_FUSED", "STAGED_MIN_NZ")
SWITCH_DEFAULTS = dict(STAGED=1, STAGED_NEAREST=1, STAGED2=1, TYPED_FUSED=1, TYPED_STAGED=1, TYPED_STAGED2=1, VECTOR_FUSED=1, STAGED_MIN_NZ=4)
PLAN_COLUMNS = ("kind", "funcType", "fast", "first", "second", "inX", "inY", "outX", "outY")
CALL_COLUMNS = ("nz", "type", "type2", "aligned", "shapes", "chunks")

NEAREST, BILINEAR, BICUBIC = 0, 1, 2  # PlanKind
# include/fimex_amd.h
FUNC_NEAREST, FUNC_BILINEAR, FUNC_BICUBIC, FUNC_COORD_NN, FUNC_COORD_NN_KD = 0, 1, 2, 3, 4
KIND_OF_FUNC = {FUNC_NEAREST: NEAREST, FUNC_BILINEAR: BILINEAR, FUNC_BICUBIC: BICUBIC, FUNC_COORD_NN: NEAREST, FUNC_COORD_NN_KD: NEAREST}  # capi_regrid.hip:56-58
CDM_NAT, CDM_CHAR, CDM_SHORT, CDM_INT, CDM_FLOAT, CDM_DOUBLE, CDM_STRING, CDM_UCHAR, CDM_USHORT, CDM_UINT, CDM_INT64, CDM_UINT64 = range(12)
SECOND, FIRST, GATHER, THREE_PASSES = 0, 1, 2, 3  # the float answer uses the first three
MAX_SLICES = 0xFFFFFFFF


def _a(x):
    return np.asarray(x)


def _is(x, *values):
    x = _a(x)
    r = np.zeros(x.shape, bool)
    for v in values:
        r = r | (x == v)
    return r


# ---------------------------------------------------------------- backward_plan.hip

def builds_first(sw, plan):
    """build_backward_plan, backward_plan.hip:110-111 (before build_staged_plan is tried)."""
    return (_a(sw["STAGED"]) != 0) & ((_a(plan["kind"]) != NEAREST) | (_a(sw["STAGED_NEAREST"]) != 0))


def builds_second(sw, plan):
    """build_backward_plan, backward_plan.hip:122-124 (`wantSecond`; plan["first"] is what :110-111 left in plan.staged.valid)."""
    second = _a(sw["STAGED2"])
    want = (second >= 2) | ((second == 1) & ((_a(plan["kind"]) != BICUBIC) | ~_a(plan["first"]).astype(bool) | _a(plan["fast"]).astype(bool)))
    return (_a(sw["STAGED"]) != 0) & want


def takes_second_form(sw, plan, nz):
    """takes_second_form, backward_plan.hip:143-147."""
    second = _a(plan["second"]).astype(bool) & ((_a(plan["kind"]) != BICUBIC) | _a(plan["fast"]).astype(bool) | ~_a(plan["first"]).astype(bool) |
                                               (_a(sw["STAGED2"]) >= 2))
    return second & (_a(sw["STAGED"]) != 0) & (_a(sw["STAGED2"]) != 0) & (_a(nz) >= _a(sw["STAGED_MIN_NZ"]))


def launch_order_is_reported(sw, plan, call):
    """backward_launch_order, backward_plan.hip:149-152: >= 0 (fimex_amd_regrid_plan_launch_order, capi_regrid.hip:272-278)."""
    return takes_second_form(sw, plan, call["nz"])


def float_apply(sw, plan, call):
    """launch_backward_apply, backward_plan.hip:154-167: SECOND, FIRST or GATHER."""
    second = takes_second_form(sw, plan, call["nz"])                                                                  # :158
    first = _a(plan["first"]).astype(bool) & (_a(sw["STAGED"]) != 0) & (_a(call["nz"]) >= _a(sw["STAGED_MIN_NZ"]))  # :162
    return np.where(second, SECOND, np.where(first, FIRST, GATHER))


def float_list(sw, plan, call):
    """launch_backward_apply_list, backward_plan.hip:190-199, without staged2_list_serves' list_shape (staged2_list.hip:53-56;
    its plan.staged2.valid is part of takes_second_form).  Backward plans only, as everything here."""
    return takes_second_form(sw, plan, call["nz"])


def _staged_types(t):
    return _is(t, CDM_CHAR, CDM_UCHAR, CDM_SHORT, CDM_USHORT)


def _elem_bytes(t):
    return np.where(_is(t, CDM_SHORT, CDM_USHORT), 2, 1)


def _typed_form_may_exist(plan, elem_bytes):
    """staged2_typed_form, staged2_typed.hip:26-27, before the form is built."""
    return _is(plan["kind"], NEAREST, BILINEAR) & ((_a(plan["inX"]) * _a(plan["inY"]) * elem_bytes) % 4 == 0)


def typed_second(sw, plan, call):
    """launch_typed_apply's first `if`, backward_plan.hip:178-180, and what launch_staged2_apply_typed refuses before it asks for the
    form, staged2_typed.hip:88-94."""
    switches = (_a(sw["TYPED_FUSED"]) != 0) & (_a(sw["STAGED"]) != 0) & (_a(sw["TYPED_STAGED"]) != 0) & (_a(sw["TYPED_STAGED2"]) != 0)
    served = _staged_types(call["type"]) & _a(call["aligned"]).astype(bool)                         # staged2_typed.hip:88-91
    return switches & (_a(call["nz"]) >= _a(sw["STAGED_MIN_NZ"])) & served & _typed_form_may_exist(plan, _elem_bytes(call["type"]))


def typed_first(sw, plan, call):
    """launch_typed_apply's second `if`, backward_plan.hip:181-184, and launch_staged_apply_typed's refusals, staged.hip:608-612."""
    switches = (_a(sw["TYPED_FUSED"]) != 0) & (_a(sw["STAGED"]) != 0) & (_a(sw["TYPED_STAGED"]) != 0)
    nearest_ok = (_a(plan["kind"]) != NEAREST) | (_a(sw["STAGED_NEAREST"]) != 0)
    served = _a(plan["first"]).astype(bool) & _staged_types(call["type"]) & _a(call["aligned"]).astype(bool)
    return switches & _a(plan["first"]).astype(bool) & (_a(call["nz"]) >= _a(sw["STAGED_MIN_NZ"])) & nearest_ok & served


def typed_gather(sw, plan, call):
    """launch_typed_apply's end, backward_plan.hip:186-187, and launch_typed_gather, gather.hip:274-279: the launcher is entered and
    does not return false.  (:278 comes before :279: more than 2^32 - 1 slices raise "too many slices" whatever the grid.)"""
    fused = _a(sw["TYPED_FUSED"])
    reached = ~((_a(plan["kind"]) == BICUBIC) & (fused < 2)) & (fused != 0)                           # :186
    types = _staged_types(call["type"]) | _is(call["type"], CDM_INT)                                  # gather.hip:274-276
    cells = np.maximum(_a(plan["inX"]) * _a(plan["inY"]), _a(plan["outX"]) * _a(plan["outY"]))
    return reached & types & ((_a(call["nz"]) > MAX_SLICES) | (8 * 4 * cells <= 0xFFFFFFFF))           # gather.hip:278-279


def typed_candidates(sw, plan, call):
    """launch_typed_apply, backward_plan.hip:171-188, as the kernels it tries in order: an int8 array [..., 4] of SECOND, FIRST,
    GATHER, each where its conditions hold, then THREE_PASSES (`return false`: apply_plan_typed_device, capi_regrid.hip:22-28),
    then -1.  A stored type's second form that could not be built falls through to the next one, as the `&&` chain does."""
    s, f, g = np.broadcast_arrays(typed_second(sw, plan, call), typed_first(sw, plan, call), typed_gather(sw, plan, call))
    slots = np.full(s.shape + (4,), -1, np.int8)
    n = np.zeros(s.shape, np.int64)
    for held, name in ((s, SECOND), (f, FIRST), (g, GATHER), (np.ones(s.shape, bool), THREE_PASSES)):
        for k in range(4):
            slots[..., k] = np.where(held & (n == k), name, slots[..., k])
        n = n + held
    return slots


def typed_list(sw, plan, call):
    """launch_typed_apply_list, backward_plan.hip:203-212, and staged2_list_typed_serves without its list_shape,
    staged2_list_typed.hip:46-61 (list_elem_bytes, then staged2_typed_form)."""
    switches = (_a(sw["TYPED_FUSED"]) != 0) & (_a(sw["STAGED"]) != 0) & (_a(sw["TYPED_STAGED"]) != 0) & (_a(sw["TYPED_STAGED2"]) != 0)   # :207-208
    return (switches & (_a(call["nz"]) >= _a(sw["STAGED_MIN_NZ"])) & _a(call["aligned"]).astype(bool) &                                # :208-211
            _staged_types(call["type"]) & _typed_form_may_exist(plan, _elem_bytes(call["type"])))


# ---------------------------------------------------------------- staged2_vector.hip, staged2_vector_typed.hip, capi_vector.hip

def vector_fused(sw, plan, call):
    """staged2_vector_serves, staged2_vector.hip:194-200 (apply_vector_pair, capi_vector.hip:23: path 1, else 0)."""
    method = _is(plan["funcType"], FUNC_NEAREST, FUNC_BILINEAR)
    return (_a(plan["second"]).astype(bool) & method & (_a(call["nz"]) >= _a(sw["STAGED_MIN_NZ"])) & (_a(sw["STAGED"]) != 0) &
            (_a(sw["STAGED2"]) != 0) & (_a(sw["VECTOR_FUSED"]) != 0))


def vector_typed_fused(sw, plan, call):
    """apply_vector_pair_typed, capi_vector.hip:40, and launch_staged2_apply_vector_typed up to the form, staged2_vector_typed.hip:264-273
    (path 2, else what vector_fused says)."""
    same = _a(call["type"]) == _a(call["type2"])                                                       # capi_vector.hip:40
    types = _is(call["type"], CDM_SHORT, CDM_USHORT)                                                   # :264
    method = _is(plan["funcType"], FUNC_NEAREST, FUNC_BILINEAR)                                        # :266
    nz = (_a(call["nz"]) >= _a(sw["STAGED_MIN_NZ"])) & (_a(call["nz"]) <= MAX_SLICES)                  # :268
    switches = ((_a(sw["STAGED"]) != 0) & (_a(sw["TYPED_FUSED"]) != 0) & (_a(sw["TYPED_STAGED"]) != 0) & (_a(sw["TYPED_STAGED2"]) != 0) &
                (_a(sw["VECTOR_FUSED"]) != 0))                                                         # :269-271
    return same & types & method & _a(call["aligned"]).astype(bool) & nz & switches & _typed_form_may_exist(plan, 2)   # :267, :272


# ---------------------------------------------------------------- capi_regrid.hip

def tune_has_choice(sw, plan, call):
    """fimex_amd_regrid_plan_tune_device goes on to time launches, capi_regrid.hip:225-227."""
    shapes = _a(call["shapes"]).astype(bool)
    orders = launch_order_is_reported(sw, plan, call) & _a(call["chunks"]).astype(bool)
    return ~((_a(call["nz"]) < _a(sw["STAGED_MIN_NZ"])) | ~_a(plan["second"]).astype(bool) | ~(shapes | orders))
