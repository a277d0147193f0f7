"""Clips on the encoder's fast paths and at scale (include/ulc_amd.h section 3), beside tests/test_gpu_clips.py whose shapes stay
below every threshold of the launch sequence.  Every comparison is byte for byte against the oracle alone (clips_testlib.ClipRef;
for the ragged call clips_testlib.ragged_plan and numpy slices of the inputs), on poisoned guarded arenas.

A. (BlockSize, nChan, nStreams, maxBlocksPerCall) = (2048, 2, 70, 8), (4096, 2, 8, 8), (2048, 1, 8, 6), (16384, 1, 4, 2): clips of
   23 blocks at the most, so a call is chunks of 8 + 8 + 7 blocks (window control pipelined beside 4, 4 and 3 transform chunks on
   the side streams, one launch sequence behind the other on one stream), of 6 + 6 + 6 + 5 (3, 3, 3, then no pipeline) or eleven
   chunks of 2 and one of 1 (k_xf_big).  The rows end at every position relative to a chunk (clips_testlib.path_case).
B. 16384 + 5 rows of (256, 1): more rows than the grid of the kernels that loop over rows.
C. ulcx_corpus_ragged_dev / _host on synthetic corpora: more files than one tile of the offsets kernel, counts no encode call
   writes, every alignment pair of the byte copy, more files than the copy kernel's grid.
tests/test_clips_capi.py checks on the CPU that the inputs have the properties these tests lean on."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import guarded_buffers as gb
import clips_testlib as ct
from ulc_testlib import synth_pcm, oracle_encode_debug
from test_gpu_clips import Call, _check_rows, _amd, _dev

pytestmark = pytest.mark.gpu
G2048x2, G4096x2, G2048x1, G16384x1 = ct.PATH_GEOMS
_gid = lambda g: f"{g[0]}x{g[1]}"
_OBJECTS = {}


def _codec(geom):
    """The geometry's encoder and decoder, made once for the module.  A create that fails is the test's failure, with the
    library's message."""
    if geom not in _OBJECTS:
        amd = _amd()
        bs, ch, streams, maxk = geom
        enc = amd.BatchEncoder(streams, ch, bs, ct.RATE, maxk)
        _OBJECTS[geom] = (enc, amd.BatchDecoder(min(streams, 8), ch, bs, maxk))       # (the decoder: the geometry's tables for the index)
    return _OBJECTS[geom]


@pytest.fixture(scope="module", autouse=True)
def _close_objects():
    yield
    for enc, dec in _OBJECTS.values():
        enc.close(); dec.close()
    _OBJECTS.clear()


def _call(geom, rows=None, **kw):
    bs, ch, streams, _ = geom
    enc, dec = _codec(geom)
    rows = list(ct.path_rows(bs, ch)) if rows is None else list(rows)
    return Call(enc, dec, bs, ch, n=len(rows), streams=streams, case=ct.path_case(bs), rows=rows, **kw)


def _refs(geom, rows=None, table=False):
    bs, ch = geom[:2]
    return ct.refs(bs, ch, table=table, case=ct.path_case(bs), rows=ct.path_rows(bs, ch) if rows is None else rows)


def _same_rows(a, b, rows, what):
    for i in rows:
        assert a.nbytes[i] == b.nbytes[i] and a.count[i] == b.count[i] and a.maxb[i] == b.maxb[i], f"{what}: row {i}: counts"
        assert a.payload[i, :a.nbytes[i]].tobytes() == b.payload[i, :b.nbytes[i]].tobytes(), f"{what}: row {i}: payload bytes"
        assert a.index[i].tobytes() == b.index[i].tobytes(), f"{what}: row {i}: index row"


# ---------------------------------------------------------------------------------------------------------------------
# A. the pipelined front end and the fast-path kernels inside a clips call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ct.PATH_GEOMS, ids=_gid)
def test_scalar_vbr_rows_over_pipelined_chunks_are_the_oracles_files(geom):
    refs = _refs(geom)
    assert [r.nb for r in refs] == [ct.PATH_BLOCKS[i] for i in ct.path_rows(*geom[:2])]
    got = _call(geom).run()
    _check_rows(got, refs, f"VBR 50 at {_gid(geom)}, chunks of {geom[3]}")
    assert got.count.tolist() == [r.nb for r in refs]


@pytest.mark.parametrize("geom", (G2048x2, G4096x2), ids=_gid)
def test_a_table_carries_the_rate_search_over_chunk_boundaries(geom):
    got = _call(geom, table=True).run()
    _check_rows(got, _refs(geom, table=True), f"per-row table at {_gid(geom)}")


def test_pcm16_over_pipelined_chunks_equals_the_float_call():
    f = _call(G2048x2).run()
    h = _call(G2048x2, pcm16=True).run()
    _check_rows(h, _refs(G2048x2), "pcm16 at 2048x2")
    _same_rows(h, f, range(7), "pcm16 vs float")


def test_rows_across_a_stream_group_and_one_row_alone():
    """65 rows on the object of 70 streams: the window-control kernels' second stream group holds one row; the call's row count
    is not the object's.  Then n = 1 on the same object."""
    rows = [i % 7 for i in range(65)]
    assert [rows[i] for i in (62, 63, 64)] == [6, 0, 1]      # the last row of the first group and the second group's only row differ
    got = _call(G2048x2, rows=rows).run()
    _check_rows(got, _refs(G2048x2, rows), "65 rows on 70 streams")
    one = _call(G2048x2, rows=[6]).run()
    _check_rows(one, _refs(G2048x2, [6]), "one row on 70 streams")
    assert one.count[0] == 23


def test_exact_path_inside_a_clips_call():
    """force_exact(2) and force_exact(1) send every second / every block through the exact (heapsort) path with its rank-slot
    groups; the bytes stay the oracle's.  ulcx_encoder_last_fallbacks reads the counter of the call's LAST launch sequence only
    (k_cplx clears it at the head of every chunk): here the 7 rows x 7 blocks of the third chunk, so the assertion is on that
    chunk - above 0, and no more than its 49 blocks."""
    enc, _ = _codec(G2048x2)
    refs = _refs(G2048x2)
    try:
        for every in (2, 1):
            enc.force_exact(every)
            got = _call(G2048x2).run()
            fb = enc.last_fallbacks()
            print(f"force_exact({every}): last_fallbacks {fb} (the last chunk has 49 blocks)")
            _check_rows(got, refs, f"force_exact({every})")
            assert 0 < fb <= 49, (every, fb)
    finally:
        enc.force_exact(0)
    _check_rows(_call(G2048x2).run(), refs, "the hook off again")


def test_streaming_state_is_untouched_by_pipelined_clips_calls():
    import torch
    bs, ch, streams, _ = G2048x2
    enc, _ = _codec(G2048x2)
    enc.reset()
    pcm = np.stack([synth_pcm(40 + s, 4 * bs, ch, ct.RATE, transient=True, seed=3) for s in range(streams)])

    def stream2(part):                                      # ulcx_encode_dev of two blocks of every stream
        d_pcm = torch.from_numpy(np.ascontiguousarray(part)).to(_dev())
        d_out = torch.zeros((streams, 2, enc.slot), dtype=torch.uint8, device=_dev())
        d_bits = torch.zeros((streams, 2), dtype=torch.int32, device=_dev())
        enc.encode_dev(d_pcm.data_ptr(), 2, d_out.data_ptr(), d_bits.data_ptr(), mode=0, p0=50.0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_bits.cpu().numpy()
    try:
        out1, bits1 = stream2(pcm[:, :2 * bs])
        a = _call(G2048x2, table=True).run()
        out2, bits2 = stream2(pcm[:, 2 * bs:])
        b = _call(G2048x2, table=True).run()
    finally:
        enc.reset()
    out, bits = np.concatenate([out1, out2], 1), np.concatenate([bits1, bits2], 1)
    for s in range(streams):
        ref = oracle_encode_debug(pcm[s], bs, ct.RATE, 0, 50.0, slot=enc.slot)
        assert np.array_equal(bits[s], ref["bits"]), (s, bits[s], ref["bits"])
        for k in range(4):
            assert np.array_equal(out[s, k, :bits[s, k] // 8], ref["out"][k, :bits[s, k] // 8]), f"stream {s} block {k}: the clips call disturbed the stream"
    _check_rows(a, _refs(G2048x2, table=True), "between streaming calls")
    _same_rows(a, b, range(7), "the second clips call")


def test_capacity_stops_a_row_inside_the_second_chunk():
    refs = _refs(G2048x2)
    whole = _call(G2048x2).run()
    pstride, istride = ct.path_cut_strides(refs)
    got = _call(G2048x2, pstride=pstride).run()
    assert got.count[6] == 10 and got.nbytes[6] == int(refs[6].sizes[:10].sum())
    _check_rows(got, refs, "payloadStride a byte short of row 6's eleventh block")
    fit = [i for i in range(7) if refs[i].kept(pstride, got.istride) == refs[i].nb]
    _same_rows(got, whole, fit, "rows that fit the payload's stride")
    got = _call(G2048x2, istride=istride).run()
    assert got.count.tolist() == [0, 3, 8, 9, 9, 9, 9]
    _check_rows(got, refs, f"indexStride {istride}")
    for i in range(4):
        assert got.nbytes[i] == whole.nbytes[i] and got.payload[i, :got.nbytes[i]].tobytes() == whole.payload[i, :whole.nbytes[i]].tobytes(), i
    for i in (4, 5, 6):
        assert got.nbytes[i] == int(refs[i].sizes[:9].sum()) and got.index[i]["ByteOffs"][9] == got.nbytes[i]


# ---------------------------------------------------------------------------------------------------------------------
# B. more rows than the grid of the row kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_more_rows_than_the_row_kernels_grid():
    bs, ch, streams, maxk = ct.GRID_GEOM
    amd = _amd()
    case = ct.grid_case(bs)
    refs = ct.refs(bs, ch, case=case)
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 4, 5]
    enc = amd.BatchEncoder(streams, ch, bs, ct.RATE, maxk)
    dec = amd.BatchDecoder(8, ch, bs, maxk)
    try:
        got = Call(enc, dec, bs, ch, n=streams, streams=streams, case=case).run()
    finally:
        enc.close(); dec.close()
    pair = np.arange(streams) % 7
    for name, have, want in (("d_indexBlocks", got.count, [r.nb for r in refs]), ("d_payloadBytes", got.nbytes, [r.payload.size for r in refs]),
                             ("d_maxBlock", got.maxb, [int(r.sizes.max()) if r.nb else 0 for r in refs])):
        bad = np.flatnonzero(have != np.array(want, np.int32)[pair])
        assert bad.size == 0, f"{name}: {bad.size} rows differ from the oracle's, first row {bad[0]} (pair {bad[0] % 7}): {have[bad[0]]}, last row {bad[-1]}"
    want = np.zeros((7, got.pstride), np.uint8)
    for i, r in enumerate(refs):
        want[i, :r.payload.size] = r.payload
    defined = np.arange(got.pstride)[None, :] < np.array([r.payload.size for r in refs])[:, None]
    bad = np.flatnonzero(((got.payload != want[pair]) & defined[pair]).any(axis=1))
    assert bad.size == 0, f"payload: {bad.size} rows differ from the oracle's, first row {bad[0]} (pair {bad[0] % 7}), last row {bad[-1]}"
    index = np.stack([r.index_row(got.istride) for r in refs])
    bad = np.flatnonzero((got.index.view(np.uint8).reshape(streams, -1) != index[pair].view(np.uint8).reshape(streams, -1)).any(axis=1))
    assert bad.size == 0, f"index: {bad.size} rows differ from the oracle's walk, first row {bad[0]} (pair {bad[0] % 7}), last row {bad[-1]}"


# ---------------------------------------------------------------------------------------------------------------------
# C. ulcx_corpus_ragged_dev on synthetic corpora
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(c, pcap, icap, what, shift=0):
    """One ulcx_corpus_ragged_dev call; d_outPayload starts `shift` bytes into a region without alignment.  Everything the call
    writes against ragged_plan and slices of the inputs; the output bytes behind the laid-out totals (and in front of the
    shifted start) keep their poison.  -> the plan."""
    import torch
    amd = _amd()
    F, stride = c.pay.shape
    istride = c.index.shape[1]
    word = lambda name, k, role, sz=4: dict(name=name, nbytes=sz * k, align=sz, role=role, guard=sz * 8, row=sz)
    specs = [dict(name="d_payload", nbytes=F * stride, align=1, role="in", guard=8 * stride, row=stride), word("d_payloadBytes", F, "in"),
             dict(name="d_index", nbytes=8 * F * istride, align=4, role="in", guard=64 * istride, row=8, rows_per_stream=istride), word("d_indexBlocks", F, "in"),
             dict(name="d_outPayload", nbytes=max(1, pcap) + 3, align=1, role="out", guard=8 * stride, row=max(1, pcap) + 3),
             word("d_payloadOffs", F + 1, "out", 8), dict(name="d_outIndex", nbytes=8 * max(1, icap), align=4, role="out", guard=64 * istride, row=8),
             word("d_indexOffs", F + 1, "out", 8), word("d_outIndexBlocks", F, "out"), word("d_need", 2, "out", 8)]
    a = gb.build(_dev(), specs)
    a.load("d_payload", c.pay); a.load("d_payloadBytes", c.nbytes); a.load("d_index", c.index); a.load("d_indexBlocks", c.blocks)
    amd.corpus_ragged_dev(F, a.ptr("d_payload"), stride, a.ptr("d_payloadBytes"), a.ptr("d_index"), istride, a.ptr("d_indexBlocks"), a.ptr("d_outPayload") + shift, pcap,
                          a.ptr("d_payloadOffs"), a.ptr("d_outIndex"), icap, a.ptr("d_indexOffs"), a.ptr("d_outIndexBlocks"), a.ptr("d_need"))
    torch.cuda.synchronize()
    a.check()
    (poffs, ioffs, oblocks, need), pay, idx = ct.ragged_expected(c, pcap, icap)
    assert pay.size == poffs[-1] <= pcap and idx.size == ioffs[-1] <= icap
    for name, dtype, want in (("d_payloadOffs", np.int64, poffs), ("d_indexOffs", np.int64, ioffs), ("d_outIndexBlocks", np.int32, oblocks), ("d_need", np.int64, need)):
        have = a.fetch(name, dtype)
        bad = np.flatnonzero(have != want)
        assert bad.size == 0, f"{what}: {name}: {bad.size} entries differ, first [{bad[0]}] = {have[bad[0]]} vs {want[bad[0]]}, last [{bad[-1]}]"
    for name, lo, data in (("d_outPayload", shift, pay), ("d_outIndex", 0, idx.view(np.uint8).reshape(-1))):
        r = a.regions[name]
        want = gb.pattern(r.off, r.nbytes).copy()
        want[lo:lo + data.size] = data
        have = a.fetch(name)
        bad = np.flatnonzero(have != want)
        if bad.size:
            edges = (poffs if name == "d_outPayload" else ioffs * 8) + lo
            f = int(np.searchsorted(edges, bad[0], "right")) - 1
            raise AssertionError(f"{what}: {name}: {bad.size} bytes differ, first at byte {bad[0] - lo} of the output (file {f} from {edges[max(f, 0)] - lo}; "
                                 f"{data.size} bytes laid out), last at {bad[-1] - lo}")
    return poffs, ioffs, oblocks, need


@pytest.mark.parametrize("F", ct.TILE_FILES)
def test_ragged_offsets_over_tiles_of_files(F):
    c = ct.corpus_tiles(F)
    for what, pcap, icap, cut in ct.tile_caps(F):
        poffs, ioffs, oblocks, _ = _ragged(c, pcap, icap, f"{F} files, {what}")
        assert (np.diff(ioffs) > 0).sum() == cut and (cut == F or (oblocks[cut:] == 0).all()), what


def test_ragged_clamps_untrusted_tables():
    c = ct.corpus_untrusted()
    need = ct.plan_of(c)[3]
    _ragged(c, int(need[0]), int(need[1]), "untrusted tables, everything fits")
    poffs = ct.plan_of(c)[0]
    _ragged(c, int(poffs[260]) - 1, int(need[1]), "untrusted tables, cut at file 259")


@pytest.mark.parametrize("shift", range(4))
def test_ragged_byte_copy_at_every_alignment_pair(shift):
    c = ct.corpus_bytecopy()
    need = ct.plan_of(c)[3]
    _ragged(c, int(need[0]), int(need[1]), f"byte copy, output shifted by {shift}", shift=shift)


def test_ragged_more_files_than_the_copy_kernels_grid():
    c = ct.corpus_many()
    need = ct.plan_of(c)[3]
    _ragged(c, int(need[0]), int(need[1]), "16387 files")


def test_ragged_host_form_on_the_byte_copy_corpus():
    c = ct.corpus_bytecopy()
    (poffs, ioffs, oblocks, need), pay, idx = ct.ragged_expected(c, ct.NO_CAP, ct.NO_CAP)
    r = _amd().corpus_ragged(c.pay, c.nbytes, c.index, c.blocks, payload_cap=int(need[0]) + 7, index_cap=int(need[1]) + 2)
    assert r["payload_offs"].tolist() == poffs.tolist() and r["index_offs"].tolist() == ioffs.tolist()
    assert r["index_blocks"].tolist() == oblocks.tolist() and r["need"].tolist() == need.tolist()
    assert r["payload"][:pay.size].tobytes() == pay.tobytes() and not r["payload"][pay.size:].any()
    assert r["index"][:idx.size].tobytes() == idx.tobytes() and not r["index"][idx.size:].view(np.uint8).any()
