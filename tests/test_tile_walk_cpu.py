"""CPU: the case table of tests/test_gpu_tile_walk.py (tests/tile_walk_ref.py) really walks -- every family that can runs workgroups of
one tile, of an even and of an odd number of tiles, launches of unequal walks and, where a launch can leave a workgroup without a tile
(per-XCD chunks, a tile count read on the device), an empty workgroup -- and the schedule it restates covers every tile once."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tile_walk_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walks(case):
    return R.schedule(R.ntiles_of(case), case.gx, case.chunked)


@pytest.mark.parametrize("ntiles,gx,chunked,lengths", [(7, 2, False, [3, 4]), (8, 3, False, [2, 3]), (17, 5, False, [3, 4]), (9, 8, False, [1, 2]),
                                                       (8, 8, True, [1]), (9, 8, True, [0, 1, 2]), (17, 8, True, [0, 2, 3]),
                                                       (41, 16, True, [0, 2, 3]), (40, 16, True, [2, 3]), (1, 1, False, [1]), (2, 1, False, [2]),
                                                       (3, 1, True, [3]), (513, 512, True, [0, 1, 2])])
def test_schedule_restates_the_kernels_rule(ntiles, gx, chunked, lengths):
    assert R.walk_lengths(ntiles, gx, chunked) == lengths
    covered = sorted(t for w in R.schedule(ntiles, gx, chunked) for t in w)
    assert covered == list(range(ntiles))


def test_plan_restates_the_launchers_branches():
    assert R.plan(101 * 128, 32, 256) == ("2x2", 101, 2)                    # 202 tiles x column blocks: the 2 x 2 layout
    assert R.plan(99 * 128, 32, 256) == ("few", 99, 4)                      # 198: one workgroup per tile, caps ignored
    assert R.plan(99 * 128, 32, 256, cap22=2, cap41=4) == ("few", 99, 4)
    assert R.plan(50 * 128, 32, 512) == ("2x2", 50, 4)
    assert R.plan(1000 * 128, 64, 256) == ("2x2", 256, 2)
    assert R.plan(1000 * 128, 64, 256, cap22=140, xcd_chunk=True) == ("2x2", 64, 2)   # 70 -> a whole number per XCD
    assert R.plan(1000 * 128, 64, 256, cap22=140) == ("2x2", 70, 2)
    assert R.plan(1000 * 128, 64, 256, cap22=100, xcd_chunk=True) == ("2x2", 50, 2)   # below 64 workgroups: as capped
    assert R.plan(17 * 128, 64, 320, cap41=15) == ("4x1", 3, 5)
    assert R.plan(2000 * 128, 64, 64) == ("4x1", 1024, 1)
    assert R.plan(17 * 128, 64, 64, narrow_below=True, cap41=8) == ("4x1", 8, 1)
    assert R.plan(17 * 128, 64, 128, narrow_below=True, cap41=8) == ("4x1", 4, 2)      # no few-tiles branch for EPI 4 / 7
    assert R.plan(17 * 128, 64, 128, epi_pooled=True, cap22=5) == ("2x2", 5, 1)        # nor for the pooled layers
    assert R.plan(17 * 128, 64, 64, epi_pooled=True)[0] == "not served"
    assert R.plan(9 * 128, 32, 64, src_pooled_k=48) == ("4x1", 9, 1)
    assert R.plan(9 * 128, 32, 64, src_pooled_k=48, cap41=2) == ("not served", 2, 1)
    assert R.plan(9 * 128, 32, 128, src_pooled_k=48, cap41=2) == ("few", 9, 2)
    assert R.plan(1000, 32, 64)[0] == R.plan(1024, 48, 64)[0] == R.plan(1024, 32, 96)[0] == "not served"


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-%dx%dx%d-gx%d%s%s" % (c.family, c.rows // 128, c.cin, c.cout, c.gx, "c" if c.chunked else "",
                                                                                   "" if c.dev_tiles is None else "-dev%d" % c.dev_tiles))
def test_every_case_is_planned_as_its_table_row_says(case):
    ntiles = R.ntiles_of(case)
    covered = sorted(t for w in walks(case) for t in w)
    assert covered == list(range(ntiles))                       # each tile exactly once
    cap22, cap41 = R.caps_of(case)
    variant, gx, ny = R.plan_of(case, cap22, cap41)
    assert gx == case.gx and gx > 0
    assert cap22 >= case.cout // 128 and cap41 >= case.cout // 64   # a smaller cap is an empty grid
    assert case.cin in (32, 64, 128) or (case.family, case.cin) == ("dense", 512)
    if case.family == "dgrad_pooled" and (case.gx * 128) % case.k:
        assert variant == "not served" and R.plan_of(case)[0] != "not served"
        return
    assert variant in ("2x2", "4x1")                            # "few": the caps would not bite
    if case.cout % 128 == 0 and not R.FAMILIES[case.family].narrow_below:
        assert variant == "2x2"
    if case.chunked:
        assert case.family == "assembled_half"                  # the only launches that set FastArgs::xcd_chunk
    if case.dev_tiles is not None:
        assert R.FAMILIES[case.family].can_be_empty and case.dev_tiles <= case.rows // 128
    if case.geom is not None:
        assert R.GEOMETRY[case.geom]["tiles"] * 128 == case.rows
    # one tile per workgroup at the default caps: what the walked launch is compared with bit for bit
    assert R.plan_of(case)[1] == case.rows // 128


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_every_family_meets_every_class_of_walk(family):
    cases = [c for c in R.CASES if c.family == family and R.plan_of(c, *R.caps_of(c))[0] != "not served"]
    assert cases
    lengths = [sorted(len(w) for w in walks(c)) for c in cases]
    every = set(n for ls in lengths for n in ls)
    assert 1 in every
    assert any(n >= 2 and n % 2 == 0 for n in every)
    assert any(n >= 3 and n % 2 == 1 for n in every)
    assert any(ls[0] != ls[-1] for ls in lengths)
    if R.FAMILIES[family].can_be_empty:
        assert 0 in every
    else:
        assert 0 not in every
    if family == "assembled_half":  # chunks of unequal length, and an empty workgroup, under the chunked schedule itself
        chunked = [sorted(len(w) for w in walks(c)) for c in cases if R.is_chunked(c)]
        assert any(ls[0] == 0 for ls in chunked) and any(len(set(ls) - {0}) > 1 for ls in chunked)
        assert any(c.chunked and not R.is_chunked(c) for c in cases)   # asked for, but gridDim.x is no multiple of 8: round-robin


def test_the_2x2_cases_are_2x2():
    two = [c for c in R.CASES if c.cout % 128 == 0 and not R.FAMILIES[c.family].epi_pooled and not R.FAMILIES[c.family].narrow_below]
    assert two and all((c.rows // 128) * (c.cout // 128) >= 200 for c in two)
    assert all(R.plan_of(c, *R.caps_of(c))[0] == "2x2" for c in two)
    assert set(c.family for c in two) >= {"dense", "dgrad", "dgrad_pooled", "dgrad_reduce", "assembled_half"}
    rounded = [c for c in two if c.cap is not None and c.chunked]  # 70 -> 64 workgroups: a whole number per XCD
    assert rounded and all(c.gx == c.cap & ~7 and c.gx >= 64 and c.gx != c.cap for c in rounded)


def test_the_default_caps_in_the_source():
    """tests/test_gpu_tile_walk.py restores these literals after every test: a changed default must fail here, not re-tune later tests."""
    src = open(os.path.join(ROOT, "votenet_amd", "csrc", "mlp_fast.hip")).read()
    assert re.search(r"^int g_fast_cap22 = %d, g_fast_cap41 = %d;$" % R.DEFAULT_CAPS, src, re.M)
    assert re.search(r"^int g_fast_xcd_chunk = 1;", src, re.M)
