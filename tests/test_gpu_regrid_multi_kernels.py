"""Every list kernel of the second staged form (staged2_list.hip, staged2_list_typed.hip) launched at least once, on every launch
layout a caller of fimex_amd_regrid_apply_multi_* can reach: both workgroup shapes, the three launch orders, stored types in
more than one z chunk, single stores forced by one output, lists cut into several launches, and every number of DMA rounds.
tests/test_gpu_regrid_multi.py holds the entry's behaviour; this module holds the kernels.

The reference is always the CPU oracle.  Nearest, bilinear and every stored type: bit for bit with identical NaN positions;
bicubic in float arithmetic: the project's stated 1e-5 of the 4 x 4 stencil's largest magnitude (BASELINE.json,
within_float_bicubic_tolerance).  run_list also holds every variable byte for byte to its own apply_device /
regrid_apply_typed_device call, which pins the variables of a bicubic-float list that come out in the reference's arithmetic, and
DeviceList.results holds the sentinel guards around every output.  Every test asserts path == 1 and, where a query exists, the
layout it was written for (plan.launch_order, info()'s tile shape and stagedCells).  Two branches have no query: the second
workgroup shape of a float plan and the single stores of a stored type.  For those the kernel trace in
profiles/staged2_list_kernels_launched.md is the proof that the kernel named below ran.

Kernel inventory.  F<S, NT, D> = staged_apply2_list<S, NT, 4, KMAX, S == 4, D> (KMAX 5 at 1024 threads, else 6);
T<S, type, pair|single, D> = staged_apply2_list_typed<S, 512, 6, type, PAIR, D>.  D = 2: product and tuning library, D = 3: tuning
library only.

  F<1, 1024, 2>  test_launch_orders_on_lists[nearest-2], test_every_dma_round_count_of_the_list_kernels[nearest-*],
                 test_a_cut_between_two_launch_orders[nearest]
  F<2, 1024, 2>  test_second_workgroup_shapes_forced[bilinear] (USE_ALT 0), test_launch_orders_on_lists[bilinear-2],
                 test_lists_cut_into_three_launches, test_every_dma_round_count_of_the_list_kernels[bilinear-*]
  F<2, 512, 2>   test_second_workgroup_shapes_forced[bilinear] (USE_ALT 1), test_every_dma_round_count_of_the_list_kernels
                 [bilinear_alt-*]; test_tuned_plans_run_lists[bilinear] where the timing chose it
  F<4, 512, 2>   test_second_workgroup_shapes_forced[bicubic_float] (USE_ALT 0), test_launch_orders_on_lists[bicubic_float-2],
                 test_bicubic_float_list_across_a_cut, test_every_dma_round_count_of_the_list_kernels[bicubic_float-*]
  F<4, 256, 2>   test_second_workgroup_shapes_forced[bicubic_float] (USE_ALT 1), test_every_dma_round_count_of_the_list_kernels
                 [bicubic_float_alt-*]; test_tuned_plans_run_lists[bicubic_float] where the timing chose it
  F<1, 1024, 3>, F<2, 1024, 3>, F<4, 512, 3>   test_launch_orders_on_lists[*-3]
  F<2, 512, 3>, F<4, 256, 3>                   test_second_workgroup_shapes_forced (STAGE2_DEPTH 3, USE_ALT 1)
  T<1 | 2, signed char | unsigned char | short | unsigned short, pair, 2>
                 test_stored_type_lists_in_four_chunks[*-0] (all eight), test_the_benchmarked_list_of_64_short_variables (short),
                 test_stored_type_list_across_a_cut (short), test_every_dma_round_count_of_the_list_kernels[short_*] (short)
  T<..., single, 2>   test_stored_type_lists_in_four_chunks[*-1 | 2 | 3]: one output off its 4-byte boundary (all eight)
  T<..., pair, 3>, T<..., single, 3>   test_stored_type_lists_in_four_chunks_ring_of_three (all sixteen)
"""
import types

import numpy as np
import pytest

import cases
import oracle
import test_gpu_regrid_multi as multi
import test_gpu_staged2_chunk_xcd as cxcd
import test_gpu_staged2_shapes as shapes
from test_gpu_regrid_multi import run_list, split, typed_fields, typed_same_as_oracle, within_float_bicubic_tolerance
from test_gpu_staged2_shapes import affine, tile_list_chunks, typed_case

gpu = pytest.mark.gpu

K = multi.K
GEOMETRY, NZ = multi.GEOMETRY, multi.NZ
SHAPE2D = (GEOMETRY[3], GEOMETRY[2])
CHUNK_MAJOR, TILE_MAJOR, CHUNK_PER_XCD = 0, 1, 2
# info()'s tile of the plan's first workgroup shape (the second one is half as wide)
TILE = {"nearest": (512, 8), "bilinear": (512, 8), "bicubic_float": (256, 8)}


@pytest.fixture(scope="module")
def fa():
    from fimex_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no gfx950 device visible"
    assert capi.REGRID_MULTI_MAX_VARS == K
    return capi


@pytest.fixture
def product_build(fa):
    was = fa.use_tuning_build(False)
    yield
    fa.use_tuning_build(was)


_float_cases = {}


def float_case(kind, nz):
    """multi.float_case, the oracle's answer computed once per kind and length"""
    if (kind, nz) not in _float_cases:
        _float_cases[kind, nz] = multi.float_case(kind, nz)
    return _float_cases[kind, nz]


def plan_for(fa, case, tile=None):
    plan = fa.RegridPlan(case.method, case.px, case.py, *case.shape, bicubic=getattr(fa, case.arith) if case.arith else None)
    info = plan.info()
    assert info["stagedCells"] > 0 and (info["tileW"], info["tileH"]) == (tile or TILE[case.kind]), info
    return plan


def check_floats(case, got, nz):
    if case.kind == "bicubic_float":
        within_float_bicubic_tolerance(case, got, sum(nz))
    else:
        multi.same_as_oracle(got, case.want[:sum(nz)], nz)


def bit_equal(a, b):
    return len(a) == len(b) and all(cases.same(g, h) for g, h in zip(a, b))


def even_split(total, n):
    """even_z_split (staged_layout.hpp): n chunks of one size, the first total % n of them one slice longer"""
    return [0] + list(np.cumsum([total // n + (1 if c < total % n else 0) for c in range(n)]))


def chunk_major_split(total, zpb, ztail):
    """float_z_chunks (staged_layout.hpp) in chunk-major order: chunks of zpb, the last 2 * zpb slices in halves of at least ztail"""
    starts, z = [], 0
    while z < total:
        rem = total - z
        size = zpb
        if ztail > 0 and rem <= 2 * zpb:
            size = max(ztail, (rem + 1) // 2)
        if size > rem or rem - size < (ztail + 1) // 2:
            size = rem
        starts.append(z)
        z += size
    return starts + [total]


def boundary_kinds(nz, starts):
    """where the inner chunk boundaries `starts[1:-1]` fall in the list nz: on a variable's boundary, inside a variable; whether a
    chunk holds three one-slice variables whole; whether a variable has slices in three chunks"""
    ends = np.cumsum(nz)
    begins = ends - np.asarray(nz)
    inner = starts[1:-1]
    on = any(b in ends for b in inner)
    inside = any(((begins < b) & (b < ends)).any() for b in inner)
    three_in_one = any(sum(1 for s, e, z in zip(begins, ends, nz) if z == 1 and c0 <= s and e <= c1) >= 3 for c0, c1 in zip(starts, starts[1:]))
    over_three = any(sum(1 for c0, c1 in zip(starts, starts[1:]) if s < c1 and c0 < e) >= 3 for s, e in zip(begins, ends))
    return on, inside, three_in_one, over_three


# ------------------------------------------------------------------------------------------------- 1. second workgroup shapes, forced
@gpu
@pytest.mark.parametrize("kind", ["bilinear", "bicubic_float"])
def test_second_workgroup_shapes_forced(fa, tuning_build, monkeypatch, kind):
    """STAGE2_USE_ALT 0 and 1 with rings of two and of three slots: 27 slices in six variables, two chunks whose boundary lies inside
    the fourth variable (the split of test_float_lists_on_the_product_build).  No query says which shape a launch ran -- info()
    describes the plan's first shape -- so that USE_ALT 1 ran the 512-thread (bilinear) and 256-thread (bicubic) kernels is shown
    by the kernel trace in profiles/staged2_list_kernels_launched.md.  Bicubic in float arithmetic: all four are bit-equal."""
    total = sum(NZ)
    starts = even_split(total, -(-total // 25))
    assert starts == [0, 14, 27] and boundary_kinds(NZ, starts)[:2] == (False, True)
    case = float_case(kind, total)
    first = None
    for depth in ("2", "3"):
        monkeypatch.setenv("FIMEX_AMD_STAGE2_DEPTH", depth)
        for alt in ("0", "1"):
            monkeypatch.setenv("FIMEX_AMD_STAGE2_USE_ALT", alt)
            plan = plan_for(fa, case)
            assert plan.launch_order(total) == TILE_MAJOR
            got, path = run_list(fa, plan, split(case.f, NZ), SHAPE2D, seed=31)
            assert path == 1, (depth, alt)
            check_floats(case, got, NZ)
            if kind == "bicubic_float":
                first = first or got
                assert bit_equal(got, first), ("the shapes differ", depth, alt)


# ------------------------------------------------------------------------------------------------- 2. second workgroup shapes, tuned
NZ_104 = NZ * 3 + (1, 5, 1, 12, 4)


@gpu
@pytest.mark.parametrize("kind", ["nearest", "bilinear", "bicubic_float"])
def test_tuned_plans_run_lists(fa, product_build, kind):
    """The product library: tune_device on an array of 104 slices -- the shortest batch that can take the chunk-per-XCD order --
    then a list of 104 slices in 23 variables through the tuned plan.  WHICH shape and order that is depends on the timing of
    this device at this moment; the choice is printed, and whatever it is the list must be the oracle's, launch_order(104) must
    agree with info(), and every variable must equal its own call."""
    import torch
    total = sum(NZ_104)
    assert total == 104 and len(NZ_104) <= K
    case = float_case(kind, total)
    plan = plan_for(fa, case)
    d_in = torch.from_numpy(case.f).cuda()
    d_out = torch.empty((total,) + SHAPE2D, dtype=torch.float32, device="cuda")
    shape = plan.tune_device(d_in.data_ptr(), total, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    order = plan.info()["launchOrder"]
    print("tuned", kind, "shape", shape, "launchOrder", order)
    assert shape in (0, 1) and order in (0, 1) and (kind != "nearest" or shape == 0)
    assert plan.info()["tileW"] == TILE[kind][0] // (2 if shape else 1)  # (after tuning info() describes the shape kept)
    assert plan.launch_order(total) == (CHUNK_PER_XCD if order else TILE_MAJOR) and plan.launch_order(total - 1) == TILE_MAJOR
    got, path = run_list(fa, plan, split(case.f, NZ_104), SHAPE2D, seed=32)
    assert path == 1
    check_floats(case, got, NZ_104)


# ------------------------------------------------------------------------------------------------- 3. launch orders on lists
# The geometry of test_gpu_staged2_chunk_xcd (320 x 240 onto 192 x 160, overshooting every side, one outlier in the first target
# rows, the target rows from 144 on below the source) on the shapes the lists have: tiles 8 rows high and, the target being 192
# wide, one tile per band.  20 bands: cohorts of 8 bands make two full band groups and a ragged one of 4; bands 18 and 19 read
# nothing; the outlier's tile is halved twice (192 -> 128 + 64 -> 64 + 64, tile_width_step 64) and the piece that holds it, columns
# 0 .. 63 of band 0, is a gather tile.
OUT_X, OUT_Y, IN_X, IN_Y = cxcd.OUT_X, cxcd.OUT_Y, cxcd.IN_X, cxcd.IN_Y
SHAPE2D_XCD = (OUT_Y, OUT_X)
# (STAGE2_ORDER, STAGE2_ZPB, STAGE2_ZTAIL, order the launch takes, chunks, the variables)
ORDER_FORMS = [
    (2, 3, None, CHUNK_PER_XCD, 8, (1, 1, 1, 9, 1, 2, 1, 1)),                                   # 17 slices: chunks of 3 and 2
    (2, 2, None, CHUNK_PER_XCD, 16, (1, 1, 1, 9, 1, 2, 1, 1) + (1, 1, 5, 1, 1, 1, 3, 2, 1, 1, 1)),  # 35 slices: chunks of 3 and 2
    (2, 1, None, CHUNK_PER_XCD, 8, (1, 1, 3, 1, 2)),                                            # 8 chunks of one slice
    (0, 3, 1, CHUNK_MAJOR, 5, (1, 1, 1, 7, 1)),                                                 # 11 slices: 3, 3, 3, 1, 1
]
NZ_XCD = max(sum(f[5]) for f in ORDER_FORMS)
_xcd_cases = {}


def xcd_case(kind, nz=NZ_XCD):
    if (kind, nz) not in _xcd_cases:
        c = types.SimpleNamespace(kind=kind, shape=(IN_X, IN_Y, OUT_X, OUT_Y))
        c.method, _, c.arith = shapes.KINDS[kind]
        c.px, c.py = cxcd.positions()
        c.f = cases.field(nz, IN_Y, IN_X, seed=len(kind) + nz, extremes=False)
        c.want = oracle.interpolate_values(c.method, c.px, c.py, c.f, IN_X, IN_Y, OUT_X, OUT_Y)
        _xcd_cases[kind, nz] = c
    return _xcd_cases[kind, nz]


def order_form_starts(order, zpb, ztail, chunks, nz):
    """the z chunks of a form, from the rules of staged_layout.hpp restated"""
    total = sum(nz)
    if order == CHUNK_MAJOR:
        return chunk_major_split(total, zpb, ztail)
    # chunk_xcd_chunk_count: at most 16 chunks; 16 where the tile-major split makes more than 8 and no chunk gets shorter than
    # (zpb + 1) / 2, else 8
    if -(-total // zpb) > 16:
        zpb = -(-total // 16)
    shortest = (zpb + 1) // 2
    n = 16 if -(-total // zpb) > 8 and total // 16 >= shortest else (8 if total // 8 >= shortest else 0)
    assert n == chunks
    return even_split(total, n)


def test_the_order_forms_put_the_chunk_boundaries_where_they_should_lie():
    """CPU: each form's chunks restated, and where their boundaries fall in the list -- on a variable's boundary, inside a
    variable, one chunk that holds three one-slice variables whole (at depth 3 the source cursor is then two variables ahead), one
    variable with slices in three chunks.  Chunks of one slice cannot hold three variables: that form has the other three."""
    sizes = []
    for order, zpb, ztail, _, chunks, nz in ORDER_FORMS:
        starts = order_form_starts(order, zpb, ztail, chunks, nz)
        assert len(starts) == chunks + 1 and starts[-1] == sum(nz) and len(nz) <= K
        kinds = boundary_kinds(nz, starts)
        assert kinds == (True, True, zpb > 1, True), (nz, starts, kinds)
        sizes.append(sorted(set(np.diff(starts))))
    assert [sum(f[5]) for f in ORDER_FORMS] == [17, 35, 8, 11]
    assert sizes == [[2, 3], [2, 3], [1], [1, 3]]  # the last: chunk-major with a shortened tail, 3, 3, 3, 1, 1
    assert OUT_Y // 8 == 20 and -(-20 // 8) == 3 and 20 % 8 == 4  # two full band groups and a ragged one


@gpu
@pytest.mark.parametrize("kind", ["bilinear", "bicubic_float"])
def test_the_list_shapes_keep_the_gather_tile_and_the_undefined_bands(fa, tuning_build, kind):
    """The two facts of the geometry from the plan, as test_the_plan_itself_holds_the_gather_tile_and_the_undefined_band states
    them for 64 x 16 tiles.  Here the piece that turns into a gather tile is 64 columns wide, 64 * 1.7 = 108 cells of every source
    row of its footprint that are no longer staged, while the two cuts that lead to it add at most a 16-byte chunk and the shared
    stencil columns per row each, 2 * (4 + 3) cells: the plan with the outlier stages fewer cells.  The target rows 144 .. 159,
    bands 18 and 19, are all counted undefined."""
    case = xcd_case(kind)
    with_outlier = plan_for(fa, case).info()
    px, py = cxcd.positions(outlier=False)
    plain = fa.RegridPlan(case.method, px, py, IN_X, IN_Y, OUT_X, OUT_Y, bicubic=getattr(fa, case.arith) if case.arith else None).info()
    print("stagedCells with / without the outlier:", with_outlier["stagedCells"], plain["stagedCells"], "undefinedCells:", with_outlier["undefinedCells"])
    assert (plain["tileW"], plain["tileH"]) == TILE[kind] and 0 < with_outlier["stagedCells"] < plain["stagedCells"]
    assert with_outlier["undefinedCells"] >= 16 * OUT_X and with_outlier["undefinedCells"] >= plain["undefinedCells"]


@gpu
@pytest.mark.parametrize("depth", ["2", "3"])
@pytest.mark.parametrize("kind", ["nearest", "bilinear", "bicubic_float"])
def test_launch_orders_on_lists(fa, tuning_build, monkeypatch, kind, depth):
    """The chunk-per-XCD order with 8 chunks of 2 and 3 slices, with 16 chunks and with 8 chunks of one slice (shorter than the
    ring), and the chunk-major order with a shortened tail, on the plan's first workgroup shape with rings of two and three slots.
    launch_order() must name the order of the form.  Bicubic in float arithmetic under the chunk-per-XCD order is bit-equal to the
    same list under the tile-major order."""
    case = xcd_case(kind)
    monkeypatch.setenv("FIMEX_AMD_STAGE2_DEPTH", depth)
    plan = plan_for(fa, case)
    for order, zpb, ztail, runs, chunks, nz in ORDER_FORMS:
        total = sum(nz)
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ZPB", str(zpb))
        if ztail is not None:
            monkeypatch.setenv("FIMEX_AMD_STAGE2_ZTAIL", str(ztail))
        long = int(np.argmax(nz))  # the longest variable shares the pool: the separate allocations stay small
        placing = dict(seed=33, pooled=(long, long + 1))
        before = None
        if kind == "bicubic_float" and order == CHUNK_PER_XCD:
            monkeypatch.setenv("FIMEX_AMD_STAGE2_ORDER", "1")
            assert plan.launch_order(total) == TILE_MAJOR
            before, path = run_list(fa, plan, split(case.f[:total], nz), SHAPE2D_XCD, **placing)
            assert path == 1
        monkeypatch.setenv("FIMEX_AMD_STAGE2_ORDER", str(order))
        assert plan.launch_order(total) == runs, (order, zpb, total)
        got, path = run_list(fa, plan, split(case.f[:total], nz), SHAPE2D_XCD, **placing)
        assert path == 1, (order, zpb, total)
        check_floats(case, got, nz)
        assert before is None or bit_equal(got, before), ("the two orders differ", zpb, total)
        monkeypatch.delenv("FIMEX_AMD_STAGE2_ZTAIL", raising=False)


# ------------------------------------------------------------------------------------------------- 4. stored types
TYPES = [np.int8, np.uint8, np.int16, np.uint16]
NZ_TYPED = (1, 1, 1, 9, 1, 1, 1, 1, 1, 3, 2, 4)  # 26 slices
MISALIGNED = 3  # the variable whose output is moved: nine slices over the first chunk boundary, an allocation of its own
_typed_lists = {}


def typed_chunk_count(total, zpb=50):
    """typed_z_chunk_count (staged_layout.hpp)"""
    if -(-total // zpb) > 16:
        zpb = -(-total // 16)
    return max(-(-total // zpb), min(4, total // 6), 1)


def typed_list(dt, method, nz, outX=384):
    """the tiles of shapes.typed_case (a gather tile, a tile row without chunks) with variables of typed_fields"""
    key = (np.dtype(dt).name, method, nz, outX)
    if key not in _typed_lists:
        px, py, inX, inY, outY = typed_case(dt, method, outX)[:5]
        fields, bads = typed_fields(dt, inX, inY, nz, seed=len(nz) + np.dtype(dt).itemsize)
        _typed_lists[key] = (px, py, inX, inY, outX, outY, fields, bads)
    return _typed_lists[key]


def run_typed_list(fa, dt, method, nz, seed, **placing):
    px, py, inX, inY, outX, outY, fields, bads = typed_list(dt, method, nz)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    got, path = run_list(fa, plan, fields, (outY, outX), seed=seed, cdm=oracle.cdm_type_of(dt), bads=bads, **placing)
    assert path == 1
    typed_same_as_oracle(got, fields, bads, method, px, py, inX, inY, outX, outY)
    return got


def shifts_of(dt):
    return (0, 2) if np.dtype(dt).itemsize == 2 else (0, 1, 3)


def four_chunk_list(fa, dt, method, shift):
    starts = even_split(sum(NZ_TYPED), typed_chunk_count(sum(NZ_TYPED)))
    assert starts == [0, 7, 14, 20, 26] and boundary_kinds(NZ_TYPED, starts)[:2] == (True, True)
    assert typed_chunk_count(7) == 1 and typed_chunk_count(23) == 3 and typed_chunk_count(24) == 4
    assert len(set(map(str, typed_list(dt, method, NZ_TYPED)[7]))) == 4  # the fill values differ
    return run_typed_list(fa, dt, method, NZ_TYPED, seed=34, out_shift={MISALIGNED: shift} if shift else None)


TYPED_CASES = [(dt, m, s) for dt in TYPES for m in (oracle.NEAREST, oracle.BILINEAR) for s in shifts_of(dt)]


@gpu
@pytest.mark.parametrize("dt,method,shift", TYPED_CASES)
def test_stored_type_lists_in_four_chunks(fa, product_build, dt, method, shift):
    """The product library's launch of 26 slices in twelve variables, each with a fill value of its own: four chunks of 7, 7, 6
    and 6 slices, one boundary inside the fourth variable and two on variable boundaries; row length 384, so a pair of results per
    store.  shift 0: every output 4-byte aligned.  shift 1, 2, 3: the fourth variable's output alone is moved that many bytes off
    its boundary, which makes the whole launch store results one by one; a pair store there would write a neighbour's element or
    the guard.  (No query says which store form ran: the kernel trace does.)"""
    four_chunk_list(fa, dt, method, shift)


@gpu
@pytest.mark.parametrize("dt,method,shift", TYPED_CASES)
def test_stored_type_lists_in_four_chunks_ring_of_three(fa, tuning_build, monkeypatch, dt, method, shift):
    """the same lists with STAGE2T_DEPTH 3: the depth-3 twin of every stored-type list kernel"""
    monkeypatch.setenv("FIMEX_AMD_STAGE2T_DEPTH", "3")
    four_chunk_list(fa, dt, method, shift)


@gpu
@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR])
def test_the_benchmarked_list_of_64_short_variables(fa, product_build, method):
    """64 variables of one slice: four chunks of 16 variables each"""
    assert even_split(64, typed_chunk_count(64)) == [0, 16, 32, 48, 64]
    run_typed_list(fa, np.int16, method, (1,) * 64, seed=35)


# ------------------------------------------------------------------------------------------------- 5. cuts
def with_empty_variables(live):
    """the list of `live` one-slice variables with variables without slices directly before, at and after the cuts behind the
    64th and the 128th of them, and as the first and the last entry; returns nz"""
    nz = []
    for i in range(live):
        if i == 0 or i % K in (K - 1, 0, 1) and i > 1:
            nz += [0, 0] if i % K == 0 else [0]
        nz.append(1)
    return tuple(nz + [0])


def test_the_empty_variables_lie_around_the_cuts():
    nz = np.array(with_empty_variables(130))
    live = np.flatnonzero(nz)
    assert nz[0] == 0 and nz[-1] == 0 and len(live) == 130
    for cut in (64, 128):
        # entries without slices between the live variables cut - 2 | cut - 1 | cut | cut + 1, two of them at the cut itself
        assert [int(live[cut + d] - live[cut + d - 1] - 1) for d in (-1, 0, 1)] == [1, 2, 1]


@gpu
@pytest.mark.parametrize("empty", [False, True])
def test_lists_cut_into_three_launches(fa, product_build, empty):
    """130 float variables of one slice, bilinear: launches of 64, 64 and 2 variables, the last one shorter than any batch the
    second form takes on its own.  empty: with variables without slices around both cuts and at both ends of the list."""
    nz = with_empty_variables(130) if empty else (1,) * 130
    live = np.flatnonzero(nz)
    case = float_case("bilinear", 130)
    plan = plan_for(fa, case)
    assert plan.launch_order(130) == TILE_MAJOR and plan.launch_order(2) == -1
    got, path = run_list(fa, plan, split(case.f, nz), SHAPE2D, seed=36, pooled=(int(live[K - 1]), int(live[K])))
    assert path == 1
    multi.same_as_oracle(got, case.want, nz)


@gpu
@pytest.mark.parametrize("method", [oracle.NEAREST, oracle.BILINEAR])
def test_stored_type_list_across_a_cut(fa, product_build, method):
    """66 int16 variables of one slice, each with its own fill value.  The 65th variable's fill value occurs in its data and in no
    other variable's, and is no other variable's fill value: a second launch that read the fill values from the list's first
    entry on would leave those cells defined."""
    dt, nz, only = np.int16, (1,) * 66, 12345
    px, py, inX, inY, outX, outY, fields, bads = typed_list(dt, method, nz)
    fields, bads = [f.copy() for f in fields], list(bads)
    for f in fields:
        f[f == only] = only + 1
    rng = np.random.default_rng(65)
    fields[K].reshape(-1)[rng.random(fields[K].size) < 0.05] = only
    bads[K] = float(only)
    assert bads.count(float(only)) == 1 and (fields[K] == only).sum() > 100 and not any((f == only).any() for i, f in enumerate(fields) if i != K)
    plan = fa.RegridPlan(method, px, py, inX, inY, outX, outY)
    got, path = run_list(fa, plan, fields, (outY, outX), seed=37, cdm=oracle.cdm_type_of(dt), bads=bads, pooled=(K - 1, K))
    assert path == 1
    typed_same_as_oracle(got, fields, bads, method, px, py, inX, inY, outX, outY)
    assert (got[K] == only).sum() > 0  # undefined results of that variable carry its own fill value


NZ_BICUBIC_CUT = tuple(1 if i % 2 == 0 else 5 for i in range(K)) + (5, 1)


@gpu
def test_bicubic_float_list_across_a_cut(fa, product_build):
    """66 variables of 1 slice (computed in the reference's arithmetic, as their own calls are) and 5 slices (float arithmetic)
    in turn, the turn broken at the cut: variables 0 and 64 differ in length, and so do 1 and 65.  A second launch whose
    exactMask counted the variables from the list's first entry would compute both in the wrong arithmetic, which the equality
    with their own calls shows."""
    nz = NZ_BICUBIC_CUT
    assert len(nz) == 66 and nz[0] != nz[K] and nz[1] != nz[K + 1] and set(nz) == {1, 5}
    case = float_case("bicubic_float", sum(nz))
    plan = plan_for(fa, case)
    got, path = run_list(fa, plan, split(case.f, nz), SHAPE2D, seed=38, pooled=(K - 1, K))
    assert path == 1
    check_floats(case, got, nz)


NZ_TWO_ORDERS = (1, 1, 1, 9, 1, 2, 1, 1) + (1,) * 56 + (1, 1)


@gpu
@pytest.mark.parametrize("kind", ["nearest", "bilinear", "bicubic_float"])
def test_a_cut_between_two_launch_orders(fa, tuning_build, monkeypatch, kind):
    """STAGE2_ORDER 2, STAGE2_ZPB 3: the first launch, 73 slices in 64 variables, takes the chunk-per-XCD order with 16 chunks; the
    second one, two variables of one slice, falls back to the tile-major order in one chunk."""
    nz = NZ_TWO_ORDERS
    assert len(nz) == K + 2 and sum(nz[:K]) == 73 and nz[K:] == (1, 1)
    for k, v in (("STAGE2_ORDER", "2"), ("STAGE2_ZPB", "3"), ("STAGED_MIN_NZ", "1")):
        monkeypatch.setenv("FIMEX_AMD_" + k, v)
    case = float_case(kind, sum(nz))
    plan = plan_for(fa, case)
    assert plan.launch_order(73) == CHUNK_PER_XCD and plan.launch_order(2) == TILE_MAJOR and plan.launch_order(sum(nz)) == CHUNK_PER_XCD
    got, path = run_list(fa, plan, split(case.f, nz), SHAPE2D, seed=39, pooled=(3, K))
    assert path == 1
    check_floats(case, got, nz)


# ------------------------------------------------------------------------------------------------- 6. DMA rounds
def needs(stencil, px, py, inX, inY):
    """classify<STENCIL> (stencil_math.hpp) restated: per target cell whether it is defined and the source columns xa .. xb and
    rows ya .. yb it reads"""
    def rnd(v):  # C's round: half away from zero
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    rx, ry = rnd(px), rnd(py)
    xin, yin = (rx >= 0) & (rx < inX), (ry >= 0) & (ry < inY)
    if stencil == 1:
        return xin & yin, rx, rx, ry, ry
    if stencil == 4:
        return (x0 >= 1) & (x0 + 2 < inX) & (y0 >= 1) & (y0 + 2 < inY), x0 - 1, x0 + 2, y0 - 1, y0 + 2
    xlin, ylin = (x0 >= 0) & (x0 + 1 < inX), (y0 >= 0) & (y0 + 1 < inY)
    return ((xlin | xin) & (ylin | yin), np.where(xlin, x0, rx), np.where(xlin, x0 + 1, rx), np.where(ylin, y0, ry), np.where(ylin, y0 + 1, ry))


def footprint_chunks(stencil, px, py, inX, inY, outX, outY, tiles, cpc):
    """tile_list_chunks for tiles that hold undefined and border cells: the chunks TileFootprint (staged_common.hpp) counts over the
    defined cells of each tile"""
    valid, xa, xb, ya, yb = (v.reshape(outY, outX) for v in needs(stencil, px, py, inX, inY))
    counts = []
    for x0, y0, w, h in tiles:
        t = (slice(y0, y0 + h), slice(x0, x0 + w))
        v, n = valid[t], 0
        assert v.any() and yb[t][v].max() - ya[t][v].min() < shapes.MAX_ROWS
        for row in range(ya[t][v].min(), yb[t][v].max() + 1):
            use = v & (ya[t] <= row) & (row <= yb[t])
            if use.any():
                lo, hi = xa[t][use].min(), xb[t][use].max()
                n += ((row * inX + lo) % cpc + hi - lo) // cpc + 1
        counts.append(int(n))
    return counts


def plain_waves(stencil, typed, px, py, inX, inY, outX, outY, tile, nt):
    """per wave of the workgroup that runs `tile` whether all its cells are interior cells of the source: defined, and for the
    2 x 2 stencil on no border branch (the kernels' plainWave).  Float kernels: lane t holds the tile's cells t + k * nt; stored
    types: cells 2 t, 2 t + 1, 2 t + 2 nt, 2 t + 2 nt + 1."""
    valid, xa, xb, ya, yb = (v.reshape(outY, outX) for v in needs(stencil, px, py, inX, inY))
    interior = valid & ((xb - xa == stencil - 1) & (yb - ya == stencil - 1))
    x0, y0, w, h = tile
    t = np.arange(nt)[:, None]
    e = (2 * t + np.array([0, 1, 2 * nt, 2 * nt + 1])) if typed else (t + nt * np.arange(4))
    ly, lx = e // w, e % w
    inside = (ly < h) & (y0 + ly < outY)
    ok = np.zeros(e.shape, bool)
    ok[inside] = interior[(y0 + ly)[inside], (x0 + lx)[inside]]
    return ok.all(axis=1).reshape(nt // 64, 64).all(axis=1)


# name -> kind of the plan / stored type, stencil, tile width, threads, KMAX, cells per chunk, switches, the switches that lift the
# cap of a slot to KMAX * threads (STAGE2_LDS_KB: the product's 79 KiB of a 512-thread shape hold 2496 chunks, five rounds)
DMA_SHAPES = {
    "nearest": ("nearest", 1, 512, 1024, 5, 4, {}, {}),
    "bilinear": ("bilinear", 2, 512, 1024, 5, 4, {}, {}),
    "bilinear_alt": ("bilinear", 2, 256, 512, 6, 4, {"STAGE2_USE_ALT": "1"}, {"STAGE2_LDS_KB": "100"}),
    "bicubic_float": ("bicubic_float", 4, 256, 512, 6, 4, {}, {"STAGE2_LDS_KB": "100"}),
    "bicubic_float_alt": ("bicubic_float", 4, 128, 256, 6, 4, {"STAGE2_USE_ALT": "1"}, {}),
    "short_nearest": (np.int16, 1, 256, 512, 6, 8, {}, {"STAGE2T_LDS_KB": "100"}),
    "short_bilinear": (np.int16, 2, 256, 512, 6, 8, {}, {"STAGE2T_LDS_KB": "100"}),
}
# ratio of source to target cells per DMA round count 1 .. KMAX (found by stepping the ratio; the CPU test holds them)
DMA_RATIOS = {
    "nearest": (0.7, 1.05, 2.05, 3.05, 4.05),
    "bilinear": (0.7, 1.05, 1.5, 1.8, 2.15),
    "bilinear_alt": (0.7, 1.05, 1.5, 1.8, 2.15, 2.7),
    "bicubic_float": (0.7, 0.9, 1.3, 1.6, 1.9, 2.15),
    "bicubic_float_alt": (0.7, 0.9, 1.3, 1.65, 1.95, 2.15),
    "short_nearest": (1.0, 2.05, 4.05, 6.05, 8.05, 10.1),
    "short_bilinear": (1.0, 1.5, 2.15, 3.25, 4.3, 5.4),
}
DMA_CASES = [(name, k + 1) for name in DMA_SHAPES for k in range(DMA_SHAPES[name][4])]
NZ_DMA = (1, 2, 1)


def dma_case(name, k):
    """a target of two tiles by two bands; the first target column lies left of the source and the last ones right of it
    (undefined), the first row on its upper border (the border branch of the 2 x 2 stencil; the 4 x 4 stencil's first row lies inside), everything else inside"""
    what, stencil, tw, nt, kmax, cpc, env, lift = DMA_SHAPES[name]
    r = DMA_RATIOS[name][k - 1]
    outX, outY = 2 * tw, 16
    ox, oy = -1.3, (1.2 if stencil == 4 else -0.3)  # (a float lane holds cells of every second row: the 4 x 4 stencil's first rows stay inside)
    inX, inY = int((outX - 1) * r + ox) // 4 * 4, int(outY * r + oy) + 8  # (stored types: slices of a multiple of 4 bytes)
    px, py = affine(outX, outY, r, ox, oy)
    tiles = [(x0, y0, tw, 8) for y0 in (0, 8) for x0 in (0, tw)]
    counts = footprint_chunks(stencil, px, py, inX, inY, outX, outY, tiles, cpc)
    env = dict(env, **(lift if k * nt > DMA_CAP[name][0] else {}))
    return types.SimpleNamespace(what=what, stencil=stencil, tw=tw, nt=nt, cpc=cpc, env=env, px=px, py=py, shape=(inX, inY, outX, outY),
                                 tiles=tiles, counts=counts, typed=not isinstance(what, str))


# the cap of a tile's chunks (tile_chunk_cap): of the product's LDS, and with the switch that lifts it
DMA_CAP = {"nearest": (5056, 5056), "bilinear": (5056, 5056), "bilinear_alt": (2496, 3072), "bicubic_float": (2496, 3072),
           "bicubic_float_alt": (1536, 1536), "short_nearest": (2496, 3072), "short_bilinear": (2496, 3072)}


def test_the_caps_of_the_dma_round_cases_are_the_layout_rules():
    import staged_layout_host as slh
    lib = slh.load()
    for name, (what, stencil, tw, nt, kmax, cpc, env, lift) in DMA_SHAPES.items():
        kb = {1024: 159, 512: 79, 256: 52}[nt]
        lifted = int(next(iter(lift.values()))) if lift else kb
        assert (lib.sl_tile_chunk_cap(kb * 1024, 2, kmax, nt, cpc), lib.sl_tile_chunk_cap(lifted * 1024, 2, kmax, nt, cpc)) == DMA_CAP[name]
        assert DMA_CAP[name][1] > (kmax - 1) * nt  # the last round count can be reached


@pytest.mark.parametrize("name,k", DMA_CASES)
def test_list_dma_round_cases_fall_into_their_buckets(name, k):
    """CPU, from the positions alone: every tile's chunk count lies in ((k - 1) * threads, k * threads] and under the slot's cap,
    and every tile has a wave of interior cells only and a wave with undefined or border cells (the two copies of the loop)."""
    c = dma_case(name, k)
    cap = DMA_CAP[name][1 if c.env.keys() & {"STAGE2_LDS_KB", "STAGE2T_LDS_KB"} else 0]
    assert len(c.counts) == 4 and all((k - 1) * c.nt < n <= min(k * c.nt, cap) for n in c.counts), (c.counts, cap)
    # footprint_chunks is tile_list_chunks where that one applies: the same tiles with every cell inside the source
    inX, inY, outX, outY = c.shape
    r = DMA_RATIOS[name][k - 1]
    px, py = affine(outX, outY, r, 1.3, 1.6)
    inside = (int(outX * r) + 8, int(outY * r) + 8, outX, outY)
    assert footprint_chunks(c.stencil, px, py, *inside, c.tiles, c.cpc) == tile_list_chunks(c.stencil, px, py, *inside, c.tiles, c.cpc)
    for tile in c.tiles:
        plain = plain_waves(c.stencil, c.typed, c.px, c.py, *c.shape, tile, c.nt)
        assert plain.any() and not plain.all(), (tile, plain)


@gpu
@pytest.mark.parametrize("name,k", DMA_CASES)
def test_every_dma_round_count_of_the_list_kernels(fa, request, monkeypatch, name, k):
    """Lists of three variables of 1, 2 and 1 slices on tiles that need k DMA rounds per slice.  Cases without a switch run the
    product library, the others the tuning library.  Float plans: info()'s stagedCells must be the chunks counted on the CPU.
    Stored types have no such query: test_list_dma_round_cases_fall_into_their_buckets is the statement, from the same footprint
    rule with 8 cells per chunk.  Bicubic in float arithmetic runs twice: variables of fewer than four slices come out in the
    reference's arithmetic, and with STAGED_MIN_NZ 1 in float arithmetic (tuning library)."""
    c = dma_case(name, k)
    request.getfixturevalue("tuning_build" if c.env or c.what == "bicubic_float" else "product_build")
    for key, v in c.env.items():
        monkeypatch.setenv("FIMEX_AMD_" + key, v)
    inX, inY, outX, outY = c.shape
    total = sum(NZ_DMA)
    if c.typed:
        method = oracle.NEAREST if c.stencil == 1 else oracle.BILINEAR
        fields, bads = typed_fields(c.what, inX, inY, NZ_DMA, seed=k)
        plan = fa.RegridPlan(method, c.px, c.py, inX, inY, outX, outY)
        got, path = run_list(fa, plan, fields, (outY, outX), seed=40, cdm=oracle.cdm_type_of(c.what), bads=bads)
        assert path == 1
        typed_same_as_oracle(got, fields, bads, method, c.px, c.py, inX, inY, outX, outY)
        return
    c.kind = c.what
    c.method, _, c.arith = shapes.KINDS[c.what]
    c.f = cases.field(total, inY, inX, seed=k, extremes=False)
    c.want = oracle.interpolate_values(c.method, c.px, c.py, c.f, inX, inY, outX, outY)
    for min_nz in ((None, "1") if c.what == "bicubic_float" else (None,)):
        if min_nz:
            monkeypatch.setenv("FIMEX_AMD_STAGED_MIN_NZ", min_nz)
        plan = plan_for(fa, c)
        info = plan.info()
        if "STAGE2_USE_ALT" not in c.env:  # (info() describes the first shape)
            assert info["stagedCells"] == 4 * sum(c.counts), (info, c.counts)
        assert plan.launch_order(total) == TILE_MAJOR
        got, path = run_list(fa, plan, split(c.f, NZ_DMA), (outY, outX), seed=41)
        assert path == 1
        check_floats(c, got, NZ_DMA)
