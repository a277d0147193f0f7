"""The window axis on the CPU: the model of tests/window_axis_testlib.py held against the oracle's runs of the streams that
tests/test_gpu_window_axis.py encodes on the GPU, and the census of what those streams reach - which WindowCtrl codes, which
forms of the transform, which boundaries of a call's launch plan have a switched block on either side.  No GPU and no library.
pytest -s prints the census (profiles/window_axis_evidence.txt is that printout, less pytest's own progress and timing lines)."""
import os
import re
import sys
import pytest

import window_axis_testlib as W

GEOS = pytest.mark.parametrize("geo", W.GEOMETRIES, ids=W.geo_id)


def _hex(cs):
    return " ".join("%02X" % c for c in sorted(cs)) or "-"


def test_the_bindings_plan_size_is_the_headers():
    """ulc_amd.FRONT_PLAN_WORDS restates ULCX_FRONT_PLAN_WORDS of include/ulc_amd.h (which ulcx_api.cpp ties to the two maxima of
    ulcx_internal.h by a static_assert): 2 + 9 cuts + 33 steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "ulc-codec_amd"))
    import ulc_amd
    header = open(os.path.join(root, "include", "ulc_amd.h")).read()
    internal = open(os.path.join(root, "ulc-codec_amd", "csrc", "ulcx_internal.h")).read()
    words = int(re.search(r"#define\s+ULCX_FRONT_PLAN_WORDS\s+(\d+)", header).group(1))
    wc_max = int(re.search(r"#define\s+ULCX_WC_MAXCH\s+(\d+)", internal).group(1))
    xf_max = int(re.search(r"#define\s+ULCX_XF_MAXCH\s+(\d+)", internal).group(1))
    assert ulc_amd.FRONT_PLAN_WORDS == words == 2 + (xf_max + 1) + (wc_max + 1)


def test_the_code_sets_of_the_model():
    """5, 9, 17, 25, 33, 41, 49, 57 codes from BlockSize 256 to 32768: 0x10, and (4 below 512, else 8) positions times the scales
    1 .. min(7, max(lgBS - 3, 6) - 5); the low nybble is 8 + scale, the position digit nSeg .. 2 nSeg - 1."""
    assert [len(W.codes(256 << i)) for i in range(8)] == [5, 9, 17, 25, 33, 41, 49, 57]
    assert W.codes(256) == {0x10, 0x49, 0x59, 0x69, 0x79}
    for i in range(8):
        bs = 256 << i
        cs = W.codes(bs) - {W.UNDEC}
        assert {W.position(c) for c in cs} == set(range(W.n_seg(bs), 2 * W.n_seg(bs)))
        assert {W.scale(c) for c in cs} == set(range(1, W.max_scale(bs) + 1)) and all(c & 8 for c in cs)
        assert all(W.PATTERNS[W.position(c)] >> 4 for c in cs), "every switched code is decimated"
        for c in cs:
            subs = W.subblocks(c, bs)
            assert sum(s for s, _ in subs) == bs and sum(t for _, t in subs) == 1


def test_the_launch_plans_of_the_model():
    """The plain plan below 6 blocks, three chunks at 6 and 7, four chunks beside four uniform steps from 8 on; at K % 4 != 0 the
    steps are uneven and do not coincide with the cuts."""
    assert W.front_plan(5, 4) == ((0, 5), (0, 5))
    assert W.front_plan(6, 4) == ((0, 1, 3, 6), (0, 1, 3, 6))
    assert W.front_plan(7, 4) == ((0, 1, 4, 7), (0, 1, 4, 7))
    assert W.front_plan(8, 4) == ((0, 1, 3, 5, 8), (0, 2, 4, 6, 8))
    assert W.front_plan(9, 4) == ((0, 1, 3, 6, 9), (0, 2, 4, 6, 9))
    assert W.front_plan(11, 4) == ((0, 1, 4, 7, 11), (0, 2, 5, 8, 11))
    for K in range(1, 40):
        assert W.front_plan(K, 1) == ((0, K), (0, K)), "an object without side streams"
        cut, steps = W.front_plan(K, 4)
        for marks in (cut, steps):
            assert marks[0] == 0 and marks[-1] == K and all(a < b for a, b in zip(marks, marks[1:]))


@GEOS
def test_the_code_cases_reach_the_codes(geo):
    """Every code the oracle emits lies in codes(bs); every row of the table gives its code in one of the two blocks behind its
    event's; up to BlockSize 4096 the streams reach every code of the model, above that every position and every scale, and what
    is missing is what NOT_REACHED names - no more than a quarter of the set."""
    bs, ch = geo
    rows = W.TABLE[geo]
    wcs = W.wc_rows(W.oracle_runs("code", bs, ch))
    model = W.codes(bs)
    reached, by = {W.UNDEC}, {}
    for i, (code, pos, level, shape) in enumerate(rows):
        e = W.code_event_block(pos, level, shape)
        assert set(wcs[i]) <= model, f"{bs} x {ch} stream {i}: the oracle left the model: {_hex(set(wcs[i]) - model)}"
        assert code in wcs[i][e + 1:e + 3], f"{bs} x {ch} stream {i}: neither block behind block {e} has the table's code {code:#x}: {_hex(wcs[i])}"
        by[code] = i
        reached.update(wcs[i])
    for i, row in enumerate(wcs):
        for c in row:
            by.setdefault(c, i)
    missing = model - reached
    assert len({r[0] for r in rows}) == len(rows), "one row per code"
    assert missing == set(W.NOT_REACHED.get(geo, ())), f"{bs} x {ch}: not reached {_hex(missing)}, NOT_REACHED names {_hex(W.NOT_REACHED.get(geo, ()))}"
    assert 4 * len(missing) <= len(model)
    if bs <= W.FULL_SET_UP_TO:
        assert reached == model
    sw = reached - {W.UNDEC}
    assert {W.position(c) for c in sw} == set(range(W.n_seg(bs), 2 * W.n_seg(bs))), f"{bs} x {ch}: positions"
    assert {W.scale(c) for c in sw} == set(range(1, W.max_scale(bs) + 1)), f"{bs} x {ch}: scales"
    print(f"\n{bs} x {ch}: {len(reached)} of {len(model)} codes; not reached: {_hex(missing)}")
    print("  code <- stream (event block, pos, level, shape): " +
          ", ".join("%02X <- %d (%d, %d, %d, %s)" % ((c, by[c], W.code_event_block(*rows[by[c]][1:])) + rows[by[c]][1:3] + (W.shape_name(rows[by[c]][3]),)) for c in sorted(sw)))


def _census(geo, pcm16):
    bs, ch = geo
    seen, clamps = {}, {}
    for kind in ("code", "neighbour"):
        for s, row in enumerate(W.wc_rows(W.oracle_runs(kind, bs, ch))):
            assert set(row) <= W.codes(bs), f"{bs} x {ch} {kind} stream {s}: the oracle left the model"
            for k, cls in enumerate(W.classes_of(row, bs, W.CODE_K, pcm16)):
                seen.setdefault(cls, (kind, s, k))
            for k in range(1, len(row)):
                for c in W.clamp_kinds(row[k - 1], row[k], bs):
                    clamps.setdefault(c, (kind, s, k))
    return seen, clamps


@GEOS
def test_every_block_class_occurs(geo):
    """The four un-decimated forms, a decimated block with and without a switched neighbour on either side, and two switched
    blocks in a row in both orders of sub-block size: all of them at every geometry, but for what NO_CLAMP names at BlockSize
    256.  The steady form at a block from the third on, where stereo 2048 / 4096 take xf_fast; under PCM16 ingest blocks 0 and 1 of
    a call are never steady."""
    bs, ch = geo
    seen, clamps = _census(geo, False)
    for cls in W.UNDEC_CLASSES:
        assert cls in seen, f"{bs} x {ch}: no {cls[0]} block"
    for nb in W.NEIGHBOURS:
        hit = [c for c in seen if c[0] == "decimated" and c[3:] == nb]
        assert hit, f"{bs} x {ch}: no decimated block with (switched in front, behind) = {nb}"
    assert set(clamps) == {"front", "behind"} - set(W.NO_CLAMP.get(geo, ())), f"{bs} x {ch}: two switched blocks in a row: {sorted(clamps)}"
    assert geo[0] == 256 or geo not in W.NO_CLAMP
    steady_late = [1 for kind in ("code", "neighbour") for row in W.wc_rows(W.oracle_runs(kind, bs, ch))
                   for k, cls in enumerate(W.classes_of(row, bs, W.CODE_K)) if cls == ("steady",) and k % W.CODE_K >= 2]
    assert steady_late, f"{bs} x {ch}: no steady block behind the second of a call"
    seen16, _ = _census(geo, True)
    assert ("steady_head",) in seen16 and ("steady",) in seen16
    for kind in ("code", "neighbour"):
        for row in W.wc_rows(W.oracle_runs(kind, bs, ch)):
            assert all(cls != ("steady",) for k, cls in enumerate(W.classes_of(row, bs, W.CODE_K, True)) if k % W.CODE_K < 2)
    dec = sorted({c[1:3] for c in seen if c[0] == "decimated"})
    print(f"\n{bs} x {ch}: classes (first seen at kind, stream, block)" + (" - steady is xf_fast here" if W.takes_xf_fast(("steady",), bs, ch) else ""))
    for cls in W.UNDEC_CLASSES:
        print(f"  {cls[0]}: {seen[cls]}")
    for nb in W.NEIGHBOURS:
        hit = sorted(c for c in seen if c[0] == "decimated" and c[3:] == nb)
        print(f"  decimated, switched (in front, behind) = {nb}: {len(hit)} (position, scale) pairs, first {hit[0][1:3]} at {seen[hit[0]]}")
    print(f"  decimated (position, scale) pairs: {len(dec)}; in a row, clamped by the block in front {clamps.get('front', 'not reached')}, by the block behind {clamps['behind']}")


@pytest.mark.parametrize("K", W.POSITION_KS)
@pytest.mark.parametrize("geo", W.POSITION_GEOMETRIES, ids=W.geo_id)
def test_the_position_cases_cover_the_boundaries(geo, K):
    """For every interior window-control step boundary and transform cut b of a call of K blocks, in both calls, some stream has a
    switched block at b - 1 and some stream one at b - and, because the code of block b is decided one block early (from the
    envelope of block b - 1), at b + 1 too, so that the decisions on both sides of a step boundary are switches.  The same for
    the boundary between the two calls, where at least two streams are switched on both sides.  Block 0 of the first call is the
    one exception: a fresh encoder carries 0x10 into it."""
    bs, ch = geo
    rows = W.wc_rows(W.oracle_runs("position", bs, ch, K))
    assert len(rows) == 2 * K + 2
    for row in rows:
        assert set(row) <= W.codes(bs)
    sw = [{j for j, c in enumerate(row) if W.switched(c)} for row in rows]
    who = lambda j: [s for s in range(len(rows)) if j in sw[s]]
    bnd = W.boundaries(K, W.WC_PIPE)
    assert (not bnd) == (K < 6)
    lines = []
    for call in (0, 1):
        for b, kinds in sorted(bnd.items()):
            j = call * K + b
            need = [n for n in (j - 1, j, j + 1) if 1 <= n < 2 * K]        # (block 0 of a fresh encoder carries the initial 0x10)
            for n in need:
                assert who(n), f"{bs} x {ch} K = {K} call {call}: no stream has a switched block {n - call * K} at the {'/'.join(sorted(kinds))} in front of block {b}"
            lines.append(f"  call {call} {'+'.join(sorted(kinds))} in front of block {b}: streams " + " | ".join(",".join(map(str, who(n))) for n in need))
    for n in (K - 1, K, K + 1):
        assert who(n), f"{bs} x {ch} K = {K}: no switched block {n - K} at the call boundary"
    both = [s for s in range(len(rows)) if K - 1 in sw[s] and K in sw[s]]
    assert len(both) >= 2, f"{bs} x {ch} K = {K}: streams switched on both sides of the call boundary: {both}"
    every = [j for j in range(1, 2 * K) if not who(j)]
    assert not every, f"{bs} x {ch} K = {K}: no stream switches blocks {every}"
    cut, steps = W.front_plan(K, W.WC_PIPE)
    print(f"\n{bs} x {ch} K = {K}: cuts {cut} steps {steps}; switched on both sides of the call boundary: streams {both}")
    print("\n".join(lines))
