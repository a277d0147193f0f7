"""Corpus splice on the GPU (include/ulc_amd.h section 2: ulcx_corpus_splice_*): new files from block ranges of resident files.
Every expectation is the oracle's (tests/splice_testlib.py): the payload is the concatenation of the source blocks, the index the
oracle's walk of that concatenation, the PCM the oracle's decode of the concatenated rows - bit for bit.  Every call here writes
into poisoned buffers between guards (tests/guarded_buffers.py): nothing outside them is written, and no payload byte behind
d_outPayloadBytes[o]."""
import functools
import numpy as np
import pytest

from gpu_testlib import amd as _amd, to_dev as _t
import guarded_buffers as gb
import splice_testlib as S
from damage_testlib import kill_block, resize_block
from seek_testlib import oracle_seeds

pytestmark = pytest.mark.gpu
LAYOUTS = ("strided", "ragged")
POISON_F, POISON_I = 7.0, 7


def _src_dev(src, poffs=None, ioffs=None):
    """The source's buffers on the device, both layouts (plain tensors: inputs)."""
    d = dict(src.to_device())
    if poffs is not None:
        d["poffs"] = _t(poffs)
    if ioffs is not None:
        d["ioffs"] = _t(ioffs)
    return d


@functools.lru_cache(maxsize=None)
def _clean_dev(geom):
    return _src_dev(S.source(geom))


class Result:
    pass


def _splice(dec, src, d, layout, files, out_stride, out_istride, seg_offs=None, max_block=True, sync=True):
    """One ulcx_corpus_splice_dev / _ragged_dev call on poisoned, guarded outputs -> Result: payload [nOut][out_stride], nbytes,
    max_block, index [nOut][out_istride], count, seg_start as numpy, the payload region's poison, and the arena (alive: a crop
    call may read the outputs in place)."""
    offs, seg = S.seg_arrays(files)
    offs = offs if seg_offs is None else np.asarray(seg_offs, np.int32)
    n_out, n_seg = len(offs) - 1, len(seg)
    d_offs, d_seg = _t(offs), _t(seg.view(np.int32))
    a = gb.build("cuda:0", [dict(name="opay", nbytes=n_out * out_stride, align=1, role="out", row=out_stride),
                            dict(name="onb", nbytes=4 * n_out, align=4, role="out"), dict(name="omax", nbytes=4 * n_out, align=4, role="out"),
                            dict(name="oidx", nbytes=8 * n_out * out_istride, align=4, role="out", row=8 * out_istride),
                            dict(name="ocnt", nbytes=4 * n_out, align=4, role="out"), dict(name="ss", nbytes=4 * n_seg, align=4, role="out")])
    out = (n_out, d_offs.data_ptr(), d_seg.data_ptr(), n_seg, a.ptr("opay"), out_stride, a.ptr("onb"), a.ptr("omax") if max_block else 0,
           a.ptr("oidx"), out_istride, a.ptr("ocnt"), a.ptr("ss"))
    if layout == "ragged":
        dec.corpus_splice_ragged_dev(src.F, d["rpay"].data_ptr(), d["rpay"].numel(), d["poffs"].data_ptr(), d["ridx"].data_ptr(), d["ridx"].numel() // 2,
                                     d["ioffs"].data_ptr(), d["cnt"].data_ptr(), *out)
    else:
        dec.corpus_splice_dev(src.F, d["pay"].data_ptr(), src.stride, d["nb"].data_ptr(), d["idx"].data_ptr(), src.istride, d["cnt"].data_ptr(), *out)
    r = Result()
    r.arena, r.n_out, r.stride, r.istride, r.keep = a, n_out, out_stride, out_istride, (d_offs, d_seg)
    if not sync:
        return r
    return _fetch(r)


def _fetch(r):
    import torch
    torch.cuda.synchronize()
    a = r.arena
    a.check()
    r.payload = a.fetch("opay").reshape(r.n_out, r.stride)
    r.nbytes, r.max_block, r.count, r.seg_start = a.fetch("onb", np.int32), a.fetch("omax", np.int32), a.fetch("ocnt", np.int32), a.fetch("ss", np.int32)
    r.index = a.fetch("oidx", S.INDEX_DTYPE).reshape(r.n_out, r.istride)
    r.poison = gb.pattern(a.regions["opay"].off, r.n_out * r.stride).reshape(r.n_out, r.stride)
    r.poison_words = {n: gb.pattern(a.regions[n].off, a.regions[n].nbytes) for n in ("omax", "ss")}
    return r


def _assert_file(r, o, e, what):
    assert int(r.count[o]) == e.n and int(r.nbytes[o]) == e.nbytes, f"{what}: {r.count[o]} blocks, {r.nbytes[o]} bytes; the rule gives {e.n}, {e.nbytes}"
    assert int(r.max_block[o]) == e.max_block, f"{what}: largest block {r.max_block[o]}, expected {e.max_block}"
    assert r.payload[o, :e.nbytes].tobytes() == e.payload.tobytes(), f"{what}: payload bytes differ from the concatenation of the source blocks"
    assert r.payload[o, e.nbytes:].tobytes() == r.poison[o, e.nbytes:].tobytes(), f"{what}: bytes behind d_outPayloadBytes written"
    assert r.index[o].tobytes() == e.index.tobytes(), f"{what}: index row differs from the oracle's walk of the output payload:\n{r.index[o]}\n{e.index}"


def _assert_all(r, exp, starts, names, what):
    assert len(exp) == r.n_out
    for o, e in enumerate(exp):
        _assert_file(r, o, e, f"{what}, file {o} ({names[o]})")
    assert np.array_equal(r.seg_start[:len(starts)], starts), f"{what}: d_segStart {r.seg_start} vs {starts}"


def _crop(dec, r, rows, n_blocks, src):
    """ulcx_decode_crops_dev of output files `rows` from block 0, on the splice call's outputs in place -> pcm [n][n_blocks][bs][ch], bits"""
    import torch
    n = len(rows)
    d_file, d_first = _t(rows, np.int32), _t(np.zeros(n), np.int32)
    pcm = torch.full((n, n_blocks, src.bs, src.ch), POISON_F, dtype=torch.float32, device="cuda:0")
    bits = torch.full((n, n_blocks), POISON_I, dtype=torch.int32, device="cuda:0")
    a = r.arena
    dec.decode_crops_dev(r.n_out, a.ptr("opay"), r.stride, a.ptr("onb"), a.ptr("oidx"), r.istride, a.ptr("ocnt"), n, d_file.data_ptr(), d_first.data_ptr(), 0,
                         n_blocks, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), bits.cpu().numpy()


def _assert_pcm(pcm, bits, i, e, what):
    n = e.n
    assert np.array_equal(bits[i, :n], e.bits) and (bits[i, n:] == 0).all(), f"{what}: bits {bits[i]} vs the oracle's {e.bits}"
    assert pcm[i, :n].tobytes() == e.pcm.tobytes(), f"{what}: samples differ from the oracle's decode of the spliced blocks"
    assert not pcm[i, n:].any()


def _sizes(src, files):
    """Strides that hold every planned file of a call, with slack that is not a multiple of anything."""
    need_b = max(sum(max(c, 0) for _, _, c in f) for f in files)
    most = sum(int(f.nb.sum()) for f in src.files)
    return 3 * most + 37, need_b + 3


# ---------------------------------------------------------------------------------------------------------------------
# 1. the shapes of a splice
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", S.GEOMS)
def test_shapes_of_a_splice(geom, layout):
    src, d = S.source(geom), _clean_dev(geom)
    shapes = S.shapes(src)
    names, files = [n for n, _ in shapes], [f for _, f in shapes]
    stride, istride = _sizes(src, files)
    exp, starts = S.expected(src, files, stride, istride)
    assert exp[names.index("empty")].n == 0 and exp[names.index("130 one-block segments")].n == 130 and exp[names.index("file 0 three times")].n > 64
    dec = _amd().BatchDecoder(2, src.ch, src.bs, 4)
    r = _splice(dec, src, d, layout, files, stride, istride)
    _assert_all(r, exp, starts, names, f"{geom} {layout}")
    # d_outMaxBlock is optional: without it the call writes the same and leaves that buffer alone
    r2 = _splice(dec, src, d, layout, files, stride, istride, max_block=False)
    assert r2.max_block.tobytes() == r2.poison_words["omax"].tobytes()
    assert r2.index.tobytes() == r.index.tobytes() and np.array_equal(r2.nbytes, r.nbytes) and all(
        r2.payload[o, :r.nbytes[o]].tobytes() == r.payload[o, :r.nbytes[o]].tobytes() for o in range(r.n_out))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the noise chain is rebuilt, not copied
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", S.GEOMS)
def test_a_trimmed_file_decodes_as_the_oracle_decodes_its_blocks(geom, layout):
    src, d = S.source(geom), _clean_dev(geom)
    K = src.files[0].K
    files = [[(0, 5, K - 5)], [(1, 0, 3)]]
    stride, istride = _sizes(src, files)
    exp, starts = S.expected(src, files, stride, istride)
    dec = _amd().BatchDecoder(2, src.ch, src.bs, K + 1)
    r = _splice(dec, src, d, layout, files, stride, istride)
    _assert_all(r, exp, starts, ["head trim", "three blocks"], f"{geom} {layout}")
    # the states are the trimmed file's own, not the source's at those blocks
    own = oracle_seeds(src.files[0].blocks, src.ch, src.bs)
    assert (r.index["RngState"][0, 1:7] != own[6:12]).all()
    pcm, bits = _crop(dec, r, [0, 1], K - 5, src)
    for i in (0, 1):
        _assert_pcm(pcm, bits, i, exp[i], f"{geom} {layout}, file {i}")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. rung switch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rung_switch_every_block_and_every_four(layout):
    src, _ = S.switch_source()
    d = _src_dev(src)
    K = 40
    files = [S.alternate(K, 1), S.alternate(K, 4), [(1, 0, K)]]
    stride, istride = _sizes(src, files)
    exp, starts = S.expected(src, files, stride, istride)
    assert exp[0].blocks[:3] == [(0, 0), (1, 1), (0, 2)] and exp[1].blocks[3:5] == [(0, 3), (1, 4)] and all(e.n == K for e in exp)
    dec = _amd().BatchDecoder(3, 2, 2048, K + 1)
    r = _splice(dec, src, d, layout, files, stride, istride)
    _assert_all(r, exp, starts, ["every block", "every 4 blocks", "rung 1"], f"switch {layout}")
    pcm, bits = _crop(dec, r, [0, 1, 2], K, src)
    for i in range(3):
        _assert_pcm(pcm, bits, i, exp[i], f"switch {layout}, file {i}")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. capacity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", S.GEOMS)
def test_capacity_cuts_one_file_and_leaves_the_others(geom, layout):
    src, d = S.source(geom), _clean_dev(geom)
    cut_file = [(0, 0, 4), (1, 2, 3), (0, 9, 2)]             # 9 blocks: the cut inside segment 1, at its start, and between the blocks of the last one
    others = [[(1, 0, 3)], [], [(0, 2, 2), (1, 0, 1)]]
    files = [others[0], cut_file, others[1], others[2]]
    full = S.expected(src, files, 1 << 20, 64)[0]
    assert full[1].n == 9
    at = lambda n: int(sum(len(S.extent(src, f, k)) for f, k in full[1].blocks[:n]))
    big = max(e.nbytes for e in full) + 5
    dec = _amd().BatchDecoder(2, src.ch, src.bs, 4)
    base = _splice(dec, src, d, layout, files, big, 12)
    cases = [("bytes: exactly at the end of block 5", at(6), 12, 6), ("bytes: one short of the end of block 5", at(6) - 1, 12, 5),
             ("bytes: exactly at segment 1's start", at(4), 12, 4), ("bytes: one short of block 0", at(1) - 1, 12, 0),
             ("entries: one below the planned blocks", big, 9, 8), ("entries: the cut at segment 1's start", big, 5, 4),
             ("entries: inside segment 1", big, 6, 5)]
    for what, stride, istride, want in cases:
        exp, starts = S.expected(src, files, stride, istride)
        # (the others fit every capacity here but the smallest byte strides, where the rule cuts them too)
        assert exp[1].n == want, (what, exp[1].n)
        r = _splice(dec, src, d, layout, files, stride, istride)
        _assert_all(r, exp, starts, ["other", "the cut file", "empty", "other"], f"{geom} {layout}, {what}")
        assert np.array_equal(r.seg_start, base.seg_start), f"{what}: d_segStart changed by the cut"
        for o in (0, 2, 3):
            if exp[o].n == full[o].n:
                n = int(base.nbytes[o])
                assert r.nbytes[o] == n and r.payload[o, :n].tobytes() == base.payload[o, :n].tobytes() and r.count[o] == base.count[o]
                m = min(istride, 12)
                assert r.index[o, :m].tobytes() == base.index[o, :m].tobytes()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. untrusted input, device forms
# ---------------------------------------------------------------------------------------------------------------------
GOOD = [[(1, 0, 3)], [(0, 2, 2), (1, 0, 1)]]                # the output files around the bad one: untouched by it


def _around(bad):
    return [GOOD[0], bad, GOOD[1]]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", S.GEOMS)
def test_untrusted_segments(geom, layout):
    src, d = S.source(geom), _clean_dev(geom)
    K0 = src.files[0].K
    dec = _amd().BatchDecoder(2, src.ch, src.bs, 4)
    ref = _splice(dec, src, d, layout, GOOD, 1 << 16, 16)
    cases = {"File out of range": [(0, 0, 2), (2, 0, 2), (0, 4, 1)], "File negative": [(-1, 0, 2), (0, 4, 1)],
             "File out of range, no blocks": [(0, 0, 2), (7, 0, 0), (0, 4, 1)],
             "First negative": [(0, 0, 2), (0, -1, 3), (0, 4, 1)], "First past the end": [(0, 0, 2), (0, K0, 2), (0, 4, 1)],
             "First far past the end": [(0, 2 ** 31 - 1, 2 ** 31 - 1), (0, 4, 1)],
             "Count running past the end": [(0, 1, 1), (0, K0 - 2, 2 ** 31 - 1), (0, 4, 1)], "Count negative": [(0, 0, 2), (1, 3, -5), (0, 4, 1)],
             "Count negative first": [(1, 3, -(2 ** 31)), (0, 4, 1)]}
    want_n = {"File out of range": 2, "File negative": 0, "File out of range, no blocks": 3, "First negative": 2, "First past the end": 2,
              "First far past the end": 0, "Count running past the end": 3, "Count negative": 3, "Count negative first": 1}
    for what, bad in cases.items():
        files = _around(bad)
        exp, starts = S.expected(src, files, 1 << 16, 16)
        assert exp[1].n == want_n[what], (what, exp[1].n)
        r = _splice(dec, src, d, layout, files, 1 << 16, 16)
        _assert_all(r, exp, starts, ["good", what, "good"], f"{geom} {layout}, {what}")
        for o, g in ((0, 0), (2, 1)):
            assert r.index[o].tobytes() == ref.index[g].tobytes() and r.payload[o, :r.nbytes[o]].tobytes() == ref.payload[g, :ref.nbytes[g]].tobytes()
    dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_untrusted_segment_offsets(layout):
    src, d = S.source(S.STEREO), _clean_dev(S.STEREO)
    dec = _amd().BatchDecoder(2, 2, 2048, 4)
    files = [GOOD[0], [(0, 0, 2), (1, 1, 1)], GOOD[1]]       # segments 0 | 1 2 | 3 4
    exp, starts = S.expected(src, files, 1 << 16, 16)
    empty = S.expected(src, [[]], 1 << 16, 16)[0][0]
    poison = lambda r: r.poison_words["ss"].view(np.int32)
    # the last pair falls: file 2 is empty, and none of its segments exists (3 and 4 belong to nobody: not written)
    r = _splice(dec, src, d, layout, files, 1 << 16, 16, seg_offs=[0, 1, 3, 2])
    _assert_all(r, [exp[0], exp[1], empty], starts[:3], ["good", "good", "falling pair"], f"{layout}, falling")
    assert np.array_equal(r.seg_start[3:], poison(r)[3:])
    # the last pair leaves nSeg: file 2 is empty, its segments that exist get -1
    r = _splice(dec, src, d, layout, files, 1 << 16, 16, seg_offs=[0, 1, 3, 9])
    _assert_all(r, [exp[0], exp[1], empty], starts[:3], ["good", "good", "pair past nSeg"], f"{layout}, past nSeg")
    assert (r.seg_start[3:] == -1).all()
    # a negative first offset: file 0 is empty and segment 0 gets -1; the others are as ever
    r = _splice(dec, src, d, layout, files, 1 << 16, 16, seg_offs=[-2, 1, 3, 5])
    assert r.seg_start[0] == -1 and np.array_equal(r.seg_start[1:], starts[1:])
    for o, e in enumerate([empty, exp[1], exp[2]]):
        _assert_file(r, o, e, f"{layout}, negative offset, file {o}")
    dec.close()


def _with_offs(src, f, k, value):
    offs = [o.copy() for o in src.offs]
    offs[f][k] = value
    return S.source_of(src.files, offs=offs)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", S.GEOMS)
def test_untrusted_source_index(geom, layout):
    clean = S.source(geom)
    dec = _amd().BatchDecoder(2, clean.ch, clean.bs, 4)
    f0 = clean.files[0]
    K0 = f0.K
    bad_file = [(0, 2, 8), (1, 0, 2)]                         # blocks 2 .. 9 of file 0, then file 1
    files = _around(bad_file)
    ref = _splice(dec, clean, _clean_dev(geom), layout, GOOD, 1 << 16, 16)
    # GOOD reads file 0's blocks 2, 3 and file 1's 0 .. 2: the bad entries lie behind them
    for what, k, value, want in (("an entry that falls", 6, int(f0.offs[5]) - 1, 3), ("an entry equal to its predecessor", 7, int(f0.offs[6]), 4),
                                 ("a negative entry", 5, -3, 2), ("an entry outside the file", 8, int(f0.offs[-1]) + 40, 5),
                                 ("the closing entry outside the file", K0, int(f0.offs[-1]) + 1, None)):
        src = _with_offs(clean, 0, k, value)
        fl = files if want is not None else _around([(0, K0 - 3, 3), (1, 0, 2)])
        exp, starts = S.expected(src, fl, 1 << 16, 16)
        assert exp[1].n == (2 if want is None else want), (what, exp[1].n)
        r = _splice(dec, src, _src_dev(src), layout, fl, 1 << 16, 16)
        _assert_all(r, exp, starts, ["good", what, "good"], f"{geom} {layout}, {what}")
        for o, g in ((0, 0), (2, 1)):
            assert r.index[o].tobytes() == ref.index[g].tobytes() and r.nbytes[o] == ref.nbytes[g]
    dec.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", S.GEOMS)
def test_blocks_damaged_behind_the_stored_index(geom, layout):
    """A source block killed, and one resized, behind its stored index, in the first, a middle and the last place of a segment:
    the output file ends in front of it, and what it holds is still what the oracle walks."""
    clean = S.source(geom)
    dec = _amd().BatchDecoder(2, clean.ch, clean.bs, 4)
    f0 = clean.files[0]
    seeds = oracle_seeds(f0.blocks, clean.ch, clean.bs)
    ran = 0
    for kind, fn in (("kill", kill_block), ("resize", resize_block)):
        # the first block from 12 on that the damage takes out of the file (a resize may keep the block's byte count: such a
        # block is still one the rule takes; some blocks have no nybble that resizes them and leaves them alive)
        src = j = None
        for cand in range(12, 18):
            pay, _ = fn(f0.payload, f0.offs, cand, seeds, clean.ch, clean.bs)
            if pay is not None:
                s = S.source_of(clean.files, payloads=[pay, clean.files[1].payload])
                if not S.takes(s, 0, cand):
                    src, j = s, cand
                    break
        if src is None:
            continue
        assert S.takes(src, 0, j - 1) and S.takes(src, 0, j + 1), kind
        d = _src_dev(src)
        for place, seg in (("first", (0, j, 3)), ("middle", (0, j - 2, 5)), ("last", (0, j - 3, 4))):
            files = _around([(1, 4, 2), seg, (1, 0, 2)])
            exp, starts = S.expected(src, files, 1 << 16, 16)
            assert exp[1].n == 2 + (j - seg[1])
            r = _splice(dec, src, d, layout, files, 1 << 16, 16)
            _assert_all(r, exp, starts, ["good", f"{kind} in the {place} place", "good"], f"{geom} {layout}, {kind}, {place}")
            ran += 1
    assert ran >= 3
    dec.close()


@pytest.mark.parametrize("case", ("end-before-start", "end-past-total", "negative-start", "2^31-bytes", "capacity-below-blocks+1", "index-offset-past-total"))
def test_ragged_forms_bad_offset_tables(case):
    src = S.source(S.STEREO)
    po, io = src.poffs.copy(), src.ioffs.copy()
    gone = (1,)
    if case == "end-before-start":
        po[2] = po[1] - 1
    elif case == "end-past-total":
        po[2] = src.rpay.size + 1
    elif case == "negative-start":
        po[0], gone = -1, (0,)
    elif case == "2^31-bytes":
        po[2] = po[1] + 2 ** 31                             # (and past the total: refused twice over; no buffer of that size is needed)
    elif case == "capacity-below-blocks+1":
        io[2] = io[1] + src.files[1].K
    else:
        io[2] = src.ridx.size + 1
    d = _src_dev(src, po, io)
    files = [[(0, 0, 3)], [(0, 1, 2), (1, 0, 2), (0, 5, 1)], [(1, 2, 2)], [(0, 7, 1)]]
    exp, starts = S.expected(src, files, 1 << 16, 16, gone=gone)
    assert [e.n for e in exp] == ([3, 2, 0, 1] if gone == (1,) else [0, 0, 2, 0])
    dec = _amd().BatchDecoder(2, 2, 2048, 4)
    r = _splice(dec, src, d, "ragged", files, 1 << 16, 16)
    _assert_all(r, exp, starts, ["a", "b", "c", "d"], case)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. every alignment pair of the copy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_alignment_pair_of_the_copy(layout):
    src, d = S.source(S.STEREO), _clean_dev(S.STEREO)
    blocks = S.alignment_blocks()
    pairs, nbytes = S.alignment_pairs(blocks)
    assert len(pairs) == 256
    files = [[(1, 3, 1)], [(f, k, 1) for f, k in blocks], [(0, 1, 2)]]
    stride, istride = nbytes + 21, len(blocks) + 2
    exp, starts = S.expected(src, files, stride, istride)
    assert exp[1].blocks == blocks
    dec = _amd().BatchDecoder(2, 2, 2048, 4)
    r = _splice(dec, src, d, layout, files, stride, istride)
    _assert_all(r, exp, starts, ["one block", "256 alignment pairs", "two blocks"], f"alignment {layout}")
    # (the destination's own start: the arena places a byte buffer on an odd address, and each file a stride further)
    assert (r.arena.ptr("opay") + stride) % 16 != 0
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. more files than a grid
# ---------------------------------------------------------------------------------------------------------------------
def test_more_output_files_than_a_grid():
    src, d = S.source(S.MANY_GEOM), _clean_dev(S.MANY_GEOM)
    pats, which = S.many_patterns()
    files = [[pats[w]] for w in which]
    stride, istride = 3 * int(max(f.nb.max() for f in src.files)) + 5, 4
    cache = {}
    exp, starts = S.expected(src, files, stride, istride, cache)
    assert len(exp) == S.MANY_FILES and len(cache) == 24
    dec = _amd().BatchDecoder(2, src.ch, src.bs, 4)
    r = _splice(dec, src, d, "strided", files, stride, istride)
    assert np.array_equal(r.seg_start, starts) and (starts == 0).all()
    want_n, want_b = np.array([e.n for e in exp]), np.array([e.nbytes for e in exp])
    assert np.array_equal(r.count, want_n) and np.array_equal(r.nbytes, want_b) and np.array_equal(r.max_block, [e.max_block for e in exp])
    want_idx = np.stack([e.index for e in exp])
    assert r.index.tobytes() == want_idx.tobytes()
    want_pay = r.poison.copy()
    for o, e in enumerate(exp):
        want_pay[o, :e.nbytes] = e.payload
    bad = np.flatnonzero((r.payload != want_pay).any(axis=1))
    assert bad.size == 0, f"{bad.size} files differ, first {bad[:5]}"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. state and order
# ---------------------------------------------------------------------------------------------------------------------
def test_the_objects_state_is_untouched_and_a_crop_call_follows_without_synchronisation():
    """A decoder in the middle of a ulcx_decode_packed_dev sequence over its two streams, with a subset sequence under way on
    stream 1 from there: a splice call, and a crop call on its outputs enqueued straight behind it, change no byte of either
    stream's saved record; the subset sequence and the packed one continue as the oracle's sequential decodes."""
    import torch
    src, d = S.source(S.STEREO), _clean_dev(S.STEREO)
    bs, ch, B, n = 2048, 2, 2, 4
    dec = _amd().BatchDecoder(B, ch, bs, 24)
    whole = [S.expected(src, [[(f, 0, 3 * n)]], 1 << 20, 64)[0][0] for f in range(2)]

    def packed(at, what):
        pcm = torch.full((B, n, bs, ch), POISON_F, dtype=torch.float32, device="cuda:0")
        bits = torch.full((B, n), POISON_I, dtype=torch.int32, device="cuda:0")
        dec.decode_packed_dev(d["pay"].data_ptr(), src.stride, d["nb"].data_ptr(), n, pcm.data_ptr(), bits.data_ptr())
        torch.cuda.synchronize()
        for s in range(B):
            assert np.array_equal(bits.cpu().numpy()[s], whole[s].bits[at:at + n]), what
            assert pcm.cpu().numpy()[s].tobytes() == whole[s].pcm[at:at + n].tobytes(), f"{what}: stream {s}"

    def subset(at, what):
        pcm, bits = dec.decode_subset([1], src.files[1].blocks[None, at:at + 2])
        assert np.array_equal(bits[0], whole[1].bits[at:at + 2]) and pcm.reshape(2, bs, ch).tobytes() == whole[1].pcm[at:at + 2].tobytes(), what

    packed(0, "first call of the sequence")
    at_four = dec.save_streams([0, 1])
    subset(n, "subset call in front of the splice call")
    before = dec.save_streams([0, 1])
    files = [[(0, 5, 19)], S.alternate(20, 1)]
    stride, istride = _sizes(src, files)
    exp, starts = S.expected(src, files, stride, istride)
    r = _splice(dec, src, d, "strided", files, stride, istride, sync=False)
    pcm, bits = _crop(dec, r, [0, 1], 20, src)               # enqueued straight behind the splice call: no synchronisation in between
    _fetch(r)
    _assert_all(r, exp, starts, ["trim", "alternating files"], "order")
    for i in (0, 1):
        _assert_pcm(pcm, bits, i, exp[i], f"crop behind the splice call, file {i}")
    assert dec.save_streams([0, 1]).tobytes() == before.tobytes(), "a stream's saved record changed"
    subset(n + 2, "subset call behind the splice call")
    dec.load_streams([0, 1], at_four)
    packed(n, "packed sequence behind the splice call")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. host forms and refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_forms_equal_the_device_forms_and_refuse_what_they_know(layout):
    amd = _amd()
    src, d = S.source(S.STEREO), _clean_dev(S.STEREO)
    shapes = S.shapes(src)
    files = [f for _, f in shapes]
    stride, istride = _sizes(src, files)
    dec = amd.BatchDecoder(2, 2, 2048, 4)
    r = _splice(dec, src, d, layout, files, stride, istride)
    seg = S.seg_arrays(files)
    poison = np.full((len(files), stride), 0xA5, np.uint8)

    def host(segments, out=None, **kw):
        st, ist = kw.get("stride", stride), kw.get("istride", istride)
        if layout == "ragged":
            return dec.corpus_splice_ragged(src.rpay, kw.get("poffs", src.poffs), src.ridx, src.ioffs, src.count, segments, st, ist, out=out)
        return dec.corpus_splice(src.host, src.nbytes, src.index, src.count, segments, st, ist, out=out)

    out = {"payload": poison.copy(), "payload_bytes": np.full(len(files), 7, np.int32), "max_block": np.full(len(files), 7, np.int32),
           "index": np.zeros((len(files), istride), S.INDEX_DTYPE), "index_blocks": np.full(len(files), 7, np.int32), "seg_start": np.full(len(seg[1]), 7, np.int32)}
    h = host(seg, out)
    assert np.array_equal(h["payload_bytes"], r.nbytes) and np.array_equal(h["index_blocks"], r.count) and np.array_equal(h["max_block"], r.max_block)
    assert h["index"].tobytes() == r.index.tobytes() and np.array_equal(h["seg_start"], r.seg_start)
    for o in range(len(files)):
        n = int(r.nbytes[o])
        assert h["payload"][o, :n].tobytes() == r.payload[o, :n].tobytes() and (h["payload"][o, n:] == 0xA5).all()
    assert host(files)["index"].tobytes() == r.index.tobytes()       # (the list form of the binding)

    def refused(segments, why, **kw):
        keep = {k: v.copy() for k, v in out.items()}
        with pytest.raises(amd.UlcError, match=why):
            host(segments, None if "stride" in kw or "istride" in kw else out, **kw)      # (strides of their own: outputs of that shape)
        assert all(out[k].tobytes() == keep[k].tobytes() for k in out), "a refused call wrote an output"
    K0 = src.files[0].K
    refused((np.array([0, 2, 1], np.int32), seg[1][:3]), "falls")
    refused((np.array([-1, 2, 3], np.int32), seg[1][:3]), "outside 0 .. nSeg")
    refused((np.array([0, 2, 4], np.int32), seg[1][:3]), "outside 0 .. nSeg")
    refused([[(2, 0, 1)]], "names file 2 of 2")
    refused([[(0, 0, 1), (-1, 0, 1)]], "names file -1")
    refused([[(0, -1, 1)]], "from block -1")
    refused([[(0, 0, -1)]], "is -1 blocks")
    refused([[(0, K0 - 1, 2)]], f"ends at block {K0 + 1} of a file of {K0}")
    refused(files, "outIndexStride 1", istride=1)
    refused(files, "outPayloadStride 0", stride=0)
    if layout == "ragged":
        po = src.poffs.copy(); po[1] = po[2] + 1
        refused(files, "file 1 is bytes", poffs=po)
    dec.close()


def test_device_forms_refuse_before_any_device_work():
    import torch
    amd = _amd()
    src, d = S.source(S.STEREO), _clean_dev(S.STEREO)
    dec = amd.BatchDecoder(2, 2, 2048, 4)
    offs, seg = S.seg_arrays(GOOD)
    d_offs, d_seg = _t(offs), _t(seg.view(np.int32))
    n_out, n_seg, stride, istride = 2, len(seg), 1 << 12, 8
    a = gb.build("cuda:0", [dict(name="opay", nbytes=n_out * stride, align=1, role="out"), dict(name="onb", nbytes=8, align=4, role="out"),
                            dict(name="omax", nbytes=8, align=4, role="out"), dict(name="oidx", nbytes=8 * n_out * istride, align=4, role="out"),
                            dict(name="ocnt", nbytes=8, align=4, role="out"), dict(name="ss", nbytes=4 * n_seg, align=4, role="out")])
    before = a.t.cpu().numpy().copy()
    base = dict(n_files=2, pay=d["pay"].data_ptr(), stride=src.stride, nb=d["nb"].data_ptr(), idx=d["idx"].data_ptr(), istride=src.istride, cnt=d["cnt"].data_ptr(),
                n_out=n_out, so=d_offs.data_ptr(), seg=d_seg.data_ptr(), n_seg=n_seg, opay=a.ptr("opay"), ostride=stride, onb=a.ptr("onb"), omax=a.ptr("omax"),
                oidx=a.ptr("oidx"), oistride=istride, ocnt=a.ptr("ocnt"), ss=a.ptr("ss"))
    order = list(base)
    rbase = dict(base, pay=d["rpay"].data_ptr(), stride=d["rpay"].numel(), nb=d["poffs"].data_ptr(), idx=d["ridx"].data_ptr(), istride=d["ridx"].numel() // 2)

    def refused(why, ragged=False, **kw):
        args = dict(rbase if ragged else base, **kw)
        with pytest.raises(amd.UlcError, match=why):
            if ragged:
                v = [args[k] for k in order]
                dec.corpus_splice_ragged_dev(*v[:6], d["ioffs"].data_ptr() if "ioffs" not in kw else kw["ioffs"], *v[6:])
            else:
                dec.corpus_splice_dev(*[args[k] for k in order])
    for k in ("pay", "nb", "idx", "cnt", "so", "seg", "opay", "onb", "oidx", "ocnt", "ss"):
        refused("NULL pointer", **{k: 0})
        refused("NULL pointer", ragged=True, **{k: 0})
    refused("NULL pointer", ragged=True, ioffs=0)
    for k in ("nb", "idx", "cnt", "so", "seg", "onb", "omax", "oidx", "ocnt", "ss"):
        refused("not aligned to 4", **{k: base[k] + 2})
    refused("not aligned to 8", ragged=True, nb=rbase["nb"] + 4)
    refused("not aligned to 8", ragged=True, ioffs=d["ioffs"].data_ptr() + 4)
    for k in ("n_files", "n_out", "n_seg"):
        refused(r"nFiles|nOut|nSeg", **{k: 0})
        refused(r"nFiles|nOut|nSeg", ragged=True, **{k: -1})
    refused("payloadStride 0", stride=0)
    refused("indexStride 0", istride=0)
    refused("payloadTotal -1", ragged=True, stride=-1)
    refused("indexTotal -1", ragged=True, istride=-1)
    refused("outPayloadStride 0", ostride=0)
    refused("outIndexStride 1", oistride=1)
    refused("outIndexStride 1", ragged=True, oistride=1)
    # an output that overlaps the source: the payload over the source's payload and index, the index likewise
    refused("overlaps", opay=base["pay"] + src.stride - 5)
    refused("overlaps", opay=base["idx"] - n_out * stride + 1)
    refused("overlaps", oidx=base["pay"] + 2 * src.stride - 4)
    refused("overlaps", oidx=base["idx"] + 8)
    refused("overlaps", ragged=True, opay=rbase["pay"] + 64)
    torch.cuda.synchronize()
    a.check()
    assert a.t.cpu().numpy().tobytes() == before.tobytes(), "a refused call wrote an output"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. corpus.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_corpus_splice_trim_and_switch(layout):
    """CropCorpus.splice / trim / switch on a two-rung from_clips_ladder corpus of 8 short clips.  The references are the oracle's
    alone: its encodes of the clips under both rungs (clips_testlib.ClipRef) - to which the corpus's files are first held byte for
    byte - and its decodes of their spliced blocks."""
    import torch
    import corpus
    import clips_testlib as ct
    amd = _amd()
    bs, ch, n_clips, T = 2048, 2, 8, 6 * 2048
    wave = ct.wave(bs, ch, T)[[0, 1, 2, 3, 4, 5, 6, 0]]
    nb = amd.clip_blocks(bs, T)
    enc = amd.BatchEncoder(n_clips, ch, bs, 44100, 8)
    dec = amd.BatchDecoder(2 * n_clips + 1, ch, bs, nb + 1)  # (the crop calls below: every file of a result at once, whole)
    cor = corpus.CropCorpus.from_clips_ladder(enc, dec, _t(wave), rates=((amd.MODE_VBR, 50.0), (amd.MODE_VBR, 20.0)), layout=layout)
    torch.cuda.synchronize()
    refs = [ct.ClipRef(bs, ch, wave[c], (-q, 0.0)) for q in (50.0, 20.0) for c in range(n_clips)]     # file_of(rung, clip) = rung * n_clips + clip
    for c in range(n_clips):
        assert np.array_equal(refs[c].wc, refs[n_clips + c].wc) and refs[c].nb == nb       # one window control for both rungs of a clip
    if layout == "ragged":
        po, pay = cor.d_payload_offs.cpu().numpy(), cor.d_payload.cpu().numpy()
        pays = [pay[po[f]:po[f + 1]] for f in range(2 * n_clips)]
    else:
        pay, nbytes = cor.d_payload.cpu().numpy(), cor.d_payload_bytes.cpu().numpy()
        pays = [pay[f, :nbytes[f]] for f in range(2 * n_clips)]
    for f, p in enumerate(pays):
        assert p.tobytes() == refs[f].payload.tobytes(), f"file {f} of the ladder corpus is not the oracle's encode"
    files = [S.File(f"file {f}", bs, ch, r.blocks, r.bits) for f, r in enumerate(refs)]
    src = S.source_of(files)

    def compare(got, segs, what):
        exp, starts = S.expected(src, segs, 1 << 22, nb * 3 + 2)
        assert got.n_files == len(segs) and got.ragged == (layout == "ragged") and got.frozen
        n_blocks = max(e.n for e in exp)
        pcm, bits = got.crops(dec, list(range(len(segs))), [0] * len(segs), n_blocks)
        torch.cuda.synchronize()
        pcm, bits = pcm.cpu().numpy().reshape(len(segs), n_blocks, bs, ch), bits.cpu().numpy()
        cnt = got.d_index_blocks.cpu().numpy()
        for o, e in enumerate(exp):
            assert cnt[o] == e.n, (what, o)
            _assert_pcm(pcm, bits, o, e, f"{what}, file {o}")
        return starts

    segs = [[(cor.file_of(0, c), 1, 3), (cor.file_of(1, (c + 1) % n_clips), 0, 2)] for c in range(n_clips)] + [[]]
    got, seg_start = cor.splice(dec, segs)
    starts = compare(got, segs, "splice")
    assert np.array_equal(seg_start.cpu().numpy(), starts)
    first = np.arange(2 * n_clips) % 3
    got = cor.trim(dec, first, 3)
    compare(got, [[(f, int(first[f]), 3)] for f in range(2 * n_clips)], "trim")
    plan = [[(c & 1, 2), (1 - (c & 1), 1), (c & 1, nb - 3)] for c in range(n_clips)]
    got = cor.switch(dec, plan)
    compare(got, [[(cor.file_of(c & 1, c), 0, 2), (cor.file_of(1 - (c & 1), c), 2, 1), (cor.file_of(c & 1, c), 3, nb - 3)] for c in range(n_clips)], "switch")
    enc.close(); dec.close()
