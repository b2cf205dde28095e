"""tests/shared_ref.py, the model of who computes what in the shared-prefix decode attention (include/qqq_amd_shared.h), on hand-built
cases; and the case tables of tests/test_gpu_packed_layouts.py through it, so that no GPU case passes without putting through the kernel
what it is there for: jobs of several live slots, live sets with holes, splits that only begin inside a prefix, siblings whose query rows lie
in two 16-row tiles, skipped tiles.  The plan is qqq_decode_attn_shared_plan's, which assumes 256 compute units where there is no device."""
import ctypes

import pytest

import shared_ref as REF
import test_gpu_packed_layouts as PL
from shared_ref import Job

MAX_LEN = 1024


def _jobs(family, shared, pos, pack, chunk=128, max_len=MAX_LEN, G=4):
    splits = -(-max_len // chunk)
    jobs = REF.jobs(family, shared, pos, pack, chunk, splits, max_len, G)
    # every (row, split) that starts at or below the row's pos is written by exactly one job, and nothing else is
    written = sorted((r, j.split) for j in jobs for r in REF.covered(j))
    want = sorted((r, sp) for r in range(len(pos)) if 0 <= pos[r] < max_len for sp in range(splits) if sp * chunk <= pos[r])
    assert written == want
    return jobs


def test_a_lone_row_computes_every_split_up_to_its_pos_alone():
    assert _jobs([0], [0], [300], 4) == [Job(0, 0, 0, (0,), 127), Job(1, 0, 0, (0,), 255), Job(2, 0, 0, (0,), 300)]
    assert _jobs([0], [0], [0], 4) == [Job(0, 0, 0, (0,), 0)]
    assert _jobs([0], [0], [127], 4) == [Job(0, 0, 0, (0,), 127)] and len(_jobs([0], [0], [128], 4)) == 2
    # a lone row that claims a prefix shares it with itself: the same keys, one slot
    assert [j.live for j in _jobs([0], [256], [300], 4)] == [(0,)] * 3


def test_a_family_of_five_in_packs_of_four():
    """rows 0 ... 3 are the first pack, row 4 the second; shared = 256 is two splits"""
    jobs = _jobs([0] * 5, [256] * 5, [256, 300, 400, 600, 700], 4)
    joint = [j for j in jobs if len(j.live) > 1]
    assert joint == [Job(0, 0, 0, (0, 1, 2, 3), 127), Job(1, 0, 0, (0, 1, 2, 3), 255)]
    # the one-row pack takes the prefix through its own window: row 4, base 4
    assert [j for j in jobs if j.row == 4][:2] == [Job(0, 4, 4, (0,), 127), Job(1, 4, 4, (0,), 255)]
    # behind the prefix everyone is alone, up to the own pos
    assert [j for j in jobs if j.split == 2] == [Job(2, r, r, (0,), min(p, 383)) for r, p in enumerate([256, 300, 400, 600, 700])]
    assert not any(j.row in (1, 2, 3) and j.split < 2 for j in jobs)


def test_a_member_below_the_prefix_leaves_a_hole():
    """row 1 stands at key 200: what it shares is clamped to its 201 keys, one split.  Split 1 is taken by rows 0, 2, 3 (a hole at slot
    1) and by row 1 alone up to key 200."""
    jobs = _jobs([0] * 4, [384] * 4, [384, 200, 500, 1023], 4)
    assert Job(0, 0, 0, (0, 1, 2, 3), 127) in jobs and Job(1, 0, 0, (0, 2, 3), 255) in jobs and Job(1, 1, 1, (0,), 200) in jobs
    assert Job(2, 0, 0, (0, 2, 3), 383) in jobs and not any(j.row == 1 and j.split == 2 for j in jobs)
    assert [REF.has_hole(j) for j in jobs if len(j.live) > 1] == [False, True, True]
    # the first member below the prefix: the second one computes, the base stays the window's first row
    jobs = _jobs([0] * 3, [256] * 3, [130, 300, 400], 4)
    assert Job(0, 0, 0, (0, 1, 2), 127) in jobs and Job(1, 1, 0, (1, 2), 255) in jobs and REF.has_hole(Job(1, 1, 0, (1, 2), 255))
    assert Job(1, 0, 0, (0,), 130) in jobs and not any(j.row == 0 and j.split == 2 for j in jobs)
    # a member with fewer keys than one split shares nothing, whatever its descriptor says
    jobs = _jobs([0] * 3, [256] * 3, [100, 300, 400], 4)
    assert Job(0, 0, 0, (0,), 100) in jobs and Job(0, 1, 0, (1, 2), 127) in jobs and not any(j.row == 0 and j.split == 1 for j in jobs)


def test_a_prefix_that_ends_inside_a_split_is_private_there():
    jobs = _jobs([0] * 3, [192] * 3, [192, 250, 700], 4)
    assert [j for j in jobs if len(j.live) > 1] == [Job(0, 0, 0, (0, 1, 2), 127)]
    assert [j for j in jobs if j.split == 1] == [Job(1, 0, 0, (0,), 192), Job(1, 1, 1, (0,), 250), Job(1, 2, 2, (0,), 255)]
    assert REF.partly_shared_splits([192] * 3, [192, 250, 700], 128, 8, MAX_LEN) == [(0, 1), (1, 1), (2, 1)]
    # chunks of 256: the same prefix shares nothing
    assert all(j.live == (0,) for j in _jobs([0] * 3, [192] * 3, [192, 250, 700], 4, chunk=256))


def test_senseless_descriptors_make_rows_compute_alone():
    pos = [384, 400, 200, 1023, 128, 129, 600]
    alone = lambda jobs: all(j.live == (0,) and j.base == j.row for j in jobs)
    big = (1 << 63) - 1
    # forward, negative and far names; row 1 names row 0, which does not name itself; row 5 names row 4, which names row 5
    assert alone(_jobs([3, 0, -1, 99, 5, 4, 1 << 30], [384] * 7, pos, 4))
    # names of rows that are no roots: row 2 names row 1, which names row 0; row 3 names row 2
    jobs = _jobs([0, 0, 1, 2, 4, 5, 5], [384, 384, 384, 384, 128, 128, 128], pos, 4)
    assert {j.live for j in jobs if j.row in (2, 3, 4)} == {(0,)}
    assert Job(0, 5, 5, (0, 1), 127) in jobs  # rows 5 and 6 are a family of their own
    # shared beyond pos + 1 is clamped per member, below 0 shares nothing
    jobs = _jobs([0, 0, 0, 0, 4, 4, 4], [big, big, -5, -big, 1 << 40, 0, 128], pos, 4)
    assert [j for j in jobs if len(j.live) > 1] == [Job(sp, 0, 0, (0, 1), 128 * sp + 127) for sp in range(3)] + [Job(0, 4, 4, (0, 2), 127)]
    assert REF.root([0, 0, 1], 2) == 2 and REF.root([1, 1], 0) == 0 and REF.root([0, 0], 1) == 0


def test_retired_rows_take_part_in_nothing():
    for dead in (-1, MAX_LEN, MAX_LEN + 3, -(1 << 40)):
        jobs = _jobs([0] * 5, [384] * 5, [384, 390, dead, 1023, 511], 4)
        assert not any(2 in REF.covered(j) for j in jobs)
        assert Job(0, 0, 0, (0, 1, 3), 127) in jobs and Job(0, 4, 4, (0,), 127) in jobs
        # a retired first row of a pack and of a family: the next member computes
        jobs = _jobs([0] * 5, [384] * 5, [dead, 390, 700, 1023, 511], 4)
        assert Job(2, 1, 0, (1, 2, 3), 383) in jobs and not any(0 in REF.covered(j) for j in jobs)
    assert _jobs([0] * 3, [256] * 3, [-1, -1, MAX_LEN], 4) == []


def test_rows_tiles_and_straddling_slots():
    assert [REF.tiles(p, 3) for p in (5, 6, 10, 11, 21)] == [1, 2, 2, 4, 4]
    job = Job(0, 0, 0, (0, 2, 5, 10), 127)
    assert REF.query_rows(job, 3) == 33 and REF.straddling_slots(job, 3) == [5, 10] and REF.straddling_slots(job, 4) == []
    assert REF.straddling_slots(Job(0, 0, 0, tuple(range(12)), 127), 5) == [3, 6, 9] and PL.straddlers(5, 12) == [3, 6, 9]
    with pytest.raises(AssertionError):
        REF.jobs([0], [0], [0], 17, 128, 8, MAX_LEN, G=4)  # 68 query rows


# ---- the case tables of tests/test_gpu_packed_layouts.py

@pytest.fixture(scope="module")
def L():
    from qqq_amd import _lib, build

    build.build()
    return _lib.lib()


def _plan(L, b, h, kvh, pack):
    splits, chunk = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.qqq_decode_attn_shared_plan(b, h, kvh, MAX_LEN, pack, ctypes.byref(splits), ctypes.byref(chunk)) == 0
    return splits.value, chunk.value


@pytest.mark.parametrize("h,kvh,d,pack", PL.SHARED_CASES)
def test_every_shared_case_runs_what_it_is_there_for(L, h, kvh, d, pack):
    assert PL.SH.MAX_LEN == MAX_LEN
    splits, chunk = _plan(L, PL.shared_batch(pack), h, kvh, pack)
    calls = PL.check_shared_case(h, kvh, pack, splits, chunk)
    assert len(calls) == 5
    lens = PL.shared_lengths(chunk)
    assert lens[:4] == [0, chunk // 2, chunk, chunk + chunk // 2] and lens[4] % chunk == 0 and chunk < lens[4] < MAX_LEN
    for size in (0, 2, 3):  # every family size meets every length
        assert sorted(fams[size][1] for fams, _ in calls) == sorted(lens)
    assert [[n for n, _, _ in fams] for fams, _ in calls] == [[pack + 1, 1, pack, 2]] * 5


def test_the_shared_cases_cover_every_group_size_and_the_packs_of_fuse_shared(L):
    gs = {h // kvh for h, kvh, _, _ in PL.SHARED_CASES}
    assert gs == {2, 3, 5, 6, 7, 8}
    for h, kvh, _, pack in PL.SHARED_CASES:
        assert (h // kvh) * pack <= 64
    # the packs attention.py passes for a large family: min(family_max, 64 // G)
    assert {(h // kvh, pack) for h, kvh, _, pack in PL.SHARED_CASES} >= {(3, 21), (5, 12), (7, 9), (8, 8), (2, 16)}
    # every G that does not divide 16 has a case in which a sibling's rows lie in two tiles
    for G in (3, 5, 6, 7):
        assert any(h // kvh == G and PL.straddlers(G, pack) for h, kvh, _, pack in PL.SHARED_CASES), G
    # one, two and four tiles
    assert {REF.tiles(pack, h // kvh) for h, kvh, _, pack in PL.SHARED_CASES} == {1, 2, 4}


@pytest.mark.parametrize("bs", [16, 256])
@pytest.mark.parametrize("h,kvh,pack", [(24, 8, 11), (64, 8, 4)])
def test_the_partial_block_cases(L, h, kvh, pack, bs):
    splits, chunk = _plan(L, pack + 4, h, kvh, pack)
    fams = PL.check_partial_case(h, kvh, pack, bs, splits, chunk)
    assert sum(n for n, _, _ in fams) == pack + 4 and all(s % bs for n, s, _ in fams if n > 1)


@pytest.mark.parametrize("case", PL.VERIFY_CASES, ids=lambda c: "-".join(str(x) for x in c[:4]))
def test_the_verify_cases_are_what_the_table_says(case):
    PL.check_verify_case(*case)


def test_the_verify_cases_cover_every_group_size_and_combine():
    assert {c[4] for c in PL.VERIFY_CASES} == set(range(1, 9)) - {4}  # G = 4 is tests/test_gpu_verify.py's
    for G in (3, 5, 6, 7):
        assert any(c[4] == G and c[8] is not None for c in PL.VERIFY_CASES), G
    assert {c[6] for c in PL.VERIFY_CASES} == {1, 2, 4} and {c[7] for c in PL.VERIFY_CASES} == {1, 2, 4}
    for G in (2, 3, 5, 6, 8):
        assert any(h // kvh == G and t >= 3 for h, kvh, _, t in PL.VERIFY_ONE_PER_G), G
    assert (PL.V_B, PL.V_MAX_LEN) == (4, 640)
