"""The wiring of fimex_amd/csrc/backward_dispatch.hpp: every answer the library reports about which kernel served a call --
fimex_amd_regrid_plan_launch_order >= 0, the `path` of the list entries and of the pair entries -- compared with the conditions the
entry points carried before the header existed (tests/backward_dispatch_ref.py), on the tuning build, with plans built under
default and non-default switches, batches on both sides of STAGED_MIN_NZ and the call-time switches flipped one at a time.

Geometry: 320 x 18 -> 256 x 16 of test_gpu_regrid_multi.py, where both staged forms exist, and the same with 321 source columns:
no first form (it needs inX % 4 == 0) and no second form for 1-byte elements (a slice of 5778 bytes).

Results of nearest and bilinear calls are compared with the CPU oracle bit for bit, guards intact, as the neighbouring tests do
(their helpers are used); bicubic in float arithmetic keeps the 1e-5 x stencil magnitude rule of FloatCase.check.  On bicubic
plans only float lists are compared: stored types and pairs report their path.

What the rule leaves to the launchers is stated here as the tests' own facts: on these geometries every form the rule allows can
be built, and the float list kernels exist for every plan but bicubic in the reference's arithmetic (list_shape, staged2_list.hip)."""
import contextlib

import numpy as np
import pytest

import backward_dispatch_ref as ref
import cases
import oracle
import test_gpu_regrid_multi as multi
import test_gpu_staged2_shapes as shapes
import test_gpu_vector_regrid as pairs
import test_gpu_vector_regrid_typed as typed_pairs

pytestmark = pytest.mark.gpu

AFFINE = (1.3, -2.5, -1.7)  # test_gpu_regrid_multi.float_case
GEOMETRY = {"320": (320, 18, 256, 16), "321": (321, 18, 256, 16)}
for _name, (_inX, _inY, _outX, _outY) in GEOMETRY.items():  # the pair helpers look their geometries up by name
    pairs.GEOMETRY["dispatch" + _name] = ((_inX, _inY, _outX, _outY), lambda x=_outX, y=_outY: shapes.affine(x, y, *AFFINE))
    typed_pairs.GEOMETRY["dispatch" + _name] = ((_inX, _inY, _outY), lambda outX, y=_outY: shapes.affine(outX, y, *AFFINE))

# plan -> FloatCase kind, switches while the plan is built
PLANS = {"nearest": ("nearest", {}), "bilinear": ("bilinear", {}), "bicubic": ("bicubic", {}), "bicubic_float": ("bicubic_float", {}),
         "bilinear_built_with_STAGED2_0": ("bilinear", {"STAGED2": 0}), "nearest_built_with_STAGED_NEAREST_0": ("nearest", {"STAGED_NEAREST": 0})}
FLIPS = (("STAGED", 0), ("STAGED_NEAREST", 0), ("STAGED2", 0), ("STAGED2", 2), ("TYPED_FUSED", 0), ("TYPED_FUSED", 2), ("TYPED_STAGED", 0),
         ("TYPED_STAGED2", 0), ("VECTOR_FUSED", 0))
# (switches at the call, nz): both sides of both thresholds at default switches, then each switch flipped at a batch of 4
SETTINGS = [({"STAGED_MIN_NZ": m}, nz) for m in (1, 4) for nz in (3, 4)] + [({k: v}, 4) for k, v in FLIPS]
CASES = [(g, p) for g in GEOMETRY for p in PLANS]
SHAPE2D = (16, 256)
_float_cases = {}


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    return capi


@contextlib.contextmanager
def switched(monkeypatch, sw):
    with monkeypatch.context() as m:
        for k, v in sw.items():
            m.setenv("FIMEX_AMD_" + k, str(v))
        yield dict(ref.SWITCH_DEFAULTS, **sw)


def float_case(geometry, kind):
    if (geometry, kind) not in _float_cases:
        _float_cases[geometry, kind] = shapes.FloatCase(kind, *GEOMETRY[geometry], *AFFINE, nz=4)
    return _float_cases[geometry, kind]


def build(fa, monkeypatch, geometry, name):
    """(FloatCase, plan, the plan's facts as the parent's build conditions give them)"""
    kind, build_switches = PLANS[name]
    case = float_case(geometry, kind)
    inX, inY, outX, outY = case.shape
    with switched(monkeypatch, build_switches) as sw:
        plan = fa.RegridPlan(case.method, case.px, case.py, *case.shape, bicubic=getattr(fa, case.arith) if case.arith else None)
    facts = dict(kind=ref.KIND_OF_FUNC[case.method], funcType=case.method, fast=kind == "bicubic_float", first=False, second=False, inX=inX,
                 inY=inY, outX=outX, outY=outY)
    facts["first"] = bool(ref.builds_first(sw, facts)) and inX % 4 == 0  # build_staged_plan: rows of whole 16-byte chunks
    facts["second"] = bool(ref.builds_second(sw, facts))
    assert (plan.info()["stagedCells"] > 0) == (facts["first"] or facts["second"])
    return case, plan, facts


def call_facts(nz, dt=np.float32, dt2=None, aligned=True):
    return dict(nz=nz, type=oracle.cdm_type_of(dt), type2=oracle.cdm_type_of(dt2 or dt), aligned=aligned, shapes=False, chunks=False)


def run_list(plan, fields, cdm=None, bads=None, **placing):
    dl = multi.DeviceList(fields, SHAPE2D[0] * SHAPE2D[1], seed=len(fields), pooled=(), **placing)
    path = plan.apply_multi_device(dl.ins, dl.nz, dl.outs, multi._stream(), cdmType=cdm, badValue=bads)
    return dl.results(SHAPE2D), path  # (results() asserts that the guards still hold the sentinel)


@pytest.mark.parametrize("geometry,name", CASES)
def test_launch_order_and_float_lists(fa, tuning_build, monkeypatch, geometry, name):
    case, plan, facts = build(fa, monkeypatch, geometry, name)
    list_kernel = case.kind != "bicubic"  # list_shape
    seen = set()
    for switches, nz in SETTINGS:
        with switched(monkeypatch, switches) as sw:
            what = (geometry, name, switches, nz)
            call = call_facts(nz)
            assert (plan.launch_order(nz) >= 0) == bool(ref.launch_order_is_reported(sw, facts, call)), what
            parts = (1, nz - 1)
            got, path = run_list(plan, multi.split(case.f[:nz], parts))
            assert path == int(bool(ref.float_list(sw, facts, call)) and list_kernel), what
            seen.add(path)
            if case.kind == "bicubic_float":
                multi.within_float_bicubic_tolerance(case, got, nz)
            else:
                multi.same_as_oracle(got, case.want[:nz], parts)
    assert 0 in seen and (1 in seen or not (facts["second"] and list_kernel))


@pytest.mark.parametrize("geometry,name", CASES)
def test_stored_type_lists(fa, tuning_build, monkeypatch, geometry, name):
    case, plan, facts = build(fa, monkeypatch, geometry, name)
    inX, inY, outX, outY = case.shape
    compare = case.kind in ("nearest", "bilinear")
    seen = set()
    for switches, nz in SETTINGS:
        with switched(monkeypatch, switches) as sw:
            # int16, int16 with the second variable's source two bytes behind a 4-byte boundary, uint8
            for dt, shift in ((np.int16, {}), (np.int16, {1: 2}), (np.uint8, {})):
                what = (geometry, name, switches, nz, np.dtype(dt).name, shift)
                fields, bads = multi.typed_fields(dt, inX, inY, (1, nz - 1), seed=nz)
                got, path = run_list(plan, fields, cdm=oracle.cdm_type_of(dt), bads=bads, in_shift=shift)
                assert path == int(bool(ref.typed_list(sw, facts, call_facts(nz, dt, aligned=not shift)))), what
                seen.add(path)
                if compare:
                    multi.typed_same_as_oracle(got, fields, bads, case.method, case.px, case.py, inX, inY, outX, outY)
    assert 0 in seen and (1 in seen) == compare


@pytest.mark.parametrize("geometry,name", CASES)
def test_pairs(fa, tuning_build, monkeypatch, geometry, name):
    import torch
    case, plan, facts = build(fa, monkeypatch, geometry, name)
    inX, inY, outX, outY = case.shape
    vec = fa.VectorPlan(cases.rotation_matrix(outX, outY, seed=outX), outX, outY)
    compare = case.kind in ("nearest", "bilinear")
    seen = set()
    for switches, nz in SETTINGS:
        with switched(monkeypatch, switches) as sw:
            what = (geometry, name, switches, nz)
            fused = int(bool(ref.vector_fused(sw, facts, call_facts(nz))))
            u, v, _, _, wu, wv, _ = pairs._case("dispatch" + geometry, case.method, nz)
            path, d_uo, d_vo, _keep = pairs._apply(fa, plan, vec, u, v, nz)
            torch.cuda.synchronize()
            assert path == fused, what
            seen.add(path)
            if compare:
                pairs._check(d_uo.cpu().numpy(), wu, "u: ")
                pairs._check(d_vo.cpu().numpy(), wv, "v: ")
            for dtU, dtV in ((np.int16, np.int16), (np.int16, np.uint16), (np.uint8, np.uint8)):
                c = typed_pairs._case("dispatch" + geometry, outX, case.method, nz, np.dtype(dtU), np.dtype(dtV), False, "ends")
                path, b = typed_pairs._apply(fa, plan, vec, c)
                torch.cuda.synchronize()
                want = 2 if bool(ref.vector_typed_fused(sw, facts, call_facts(nz, dtU, dtV))) else fused
                assert path == want, what + (np.dtype(dtU).name, np.dtype(dtV).name)
                seen.add(path)
                if compare:
                    typed_pairs._check(b.result(0), c["wantU"], c["cmpU"], "u: ")
                    typed_pairs._check(b.result(1), c["wantV"], c["cmpV"], "v: ")
    assert 0 in seen and ({1, 2} <= seen) == (compare and facts["second"])
