"""The clips ladder call on the encoder's fast paths and at scale (include/ulc_amd.h section 3), beside
tests/test_gpu_clips_ladder.py whose shapes stay below every threshold of the launch sequence.  Every comparison is byte for byte
against the oracle alone (clips_ladder_testlib), on poisoned guarded arenas.

A. (BlockSize, nChan, nStreams, maxBlocksPerCall) = (2048, 2, 70, 8): clips of 23 blocks at the most, so each pass of the call is
   chunks of 8 + 8 + 7 blocks - the pipelined front end in the analysis pass and in the encode pass, the fast-path selection and
   writer kernels once per rung, k_rung_arm between the rungs.  Three rungs: scalar VBR 50, AUTO 64 kbps, the mixed TABLE.  Seven
   rows, then 65 rows (across a window-control stream group), then two capacities that stop the longest row's highest-rate file
   inside the second chunk.
B. 16384 + 5 rows of (256, 1) under two rungs: 2 x 16389 files, more than the grid of the kernels that loop over rows.
tests/test_clips_ladder_capi.py checks on the CPU that the inputs have the properties these tests lean on."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import clips_testlib as ct
import clips_ladder_testlib as lt
from clips_ladder_testlib import LadderCall, check_files, check_avg, _amd

pytestmark = pytest.mark.gpu
GEOM = ct.PATH_GEOMS[0]


@pytest.fixture(scope="module")
def codec():
    amd = _amd()
    bs, ch, streams, maxk = GEOM
    enc = amd.BatchEncoder(streams, ch, bs, ct.RATE, maxk)
    dec = amd.BatchDecoder(8, ch, bs, maxk)                 # (the decoder: the geometry's tables for the index)
    yield enc, dec
    enc.close(); dec.close()


def _call(codec, rows=None, **kw):
    bs, ch, streams, _ = GEOM
    rows = list(range(7)) if rows is None else list(rows)
    return LadderCall(codec[0], codec[1], bs, ch, lt.PATH_RUNGS, n=len(rows), streams=streams, case=ct.path_case(bs), rows=rows, **kw)


def _refs(rows=None):
    bs, ch = GEOM[:2]
    return lt.refs(bs, ch, lt.PATH_RUNGS, ct.path_case(bs), rows)


def test_three_rungs_over_pipelined_chunks_are_the_oracles_files(codec):
    bs, ch = GEOM[:2]
    got = _call(codec).run()
    check_files(got, _refs(), "VBR 50 | AUTO 64 | TABLE at 2048x2, chunks of 8 + 8 + 7")
    check_avg(got, bs, ch, "2048x2")
    assert got.count.reshape(3, 7).tolist() == [ct.PATH_BLOCKS] * 3


def test_rows_across_a_stream_group(codec):
    bs, ch = GEOM[:2]
    rows = [i % 7 for i in range(65)]
    got = _call(codec, rows=rows).run()
    check_files(got, _refs(rows), "65 rows on 70 streams")
    check_avg(got, bs, ch, "65 rows on 70 streams")


def test_capacities_stop_the_highest_rate_file_inside_the_second_chunk(codec):
    bs, ch = GEOM[:2]
    refs = _refs()
    hi = int(np.argmax([refs[r][6].payload.size for r in range(3)]))
    pstride, istride = ct.path_cut_strides(refs[hi])
    got = _call(codec, pstride=pstride).run()
    kept = [int(got.count[r * 7 + 6]) for r in range(3)]
    assert kept[hi] == 10 and len(set(kept)) >= 2, kept     # the rungs of row 6 stop at different blocks
    check_files(got, refs, f"payloadStride a byte short of row 6's eleventh block under rung {hi}")
    check_avg(got, bs, ch, "payload capacity")
    got = _call(codec, istride=istride).run()
    assert got.count.reshape(3, 7).tolist() == [[0, 3, 8, 9, 9, 9, 9]] * 3
    check_files(got, refs, f"indexStride {istride}")
    check_avg(got, bs, ch, "index capacity")


def test_too_many_index_entries_are_refused_and_the_object_is_as_it_was(codec):
    """8 rungs x 70 rows of 2^30 index entries are more than ulcx_index_slots_dev takes in one call: ULCX_ERR_ARG from the device
    form and from the host form before anything is allocated or enqueued (the buffers here are a few bytes), the object as it
    was - what it remembers of its last call, and the next call's files."""
    import torch
    amd = _amd()
    enc, dec = codec
    bs, ch = GEOM[:2]
    check_files(_call(codec).run(), _refs(), "the call in front")
    assert enc.last_rungs() == 3
    eight = [(0, 50.0)] * 8
    why = "560 rows of 1073741824 entries are more than one call takes"
    buf = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", 0))
    d = buf.data_ptr()
    with pytest.raises(amd.UlcError, match="ulcx_encode_clips_ladder_dev: " + why):
        enc.encode_clips_ladder_dev(dec, 70, eight, d, 0, 100, d, 64, d, d, 1 << 30, d)
    h = np.zeros(70 * ch * 100, np.float32)                 # (the host form through the C ABI: the binding would allocate the index)
    small = np.zeros(1024, np.int32)
    rc = amd.lib().ulcx_encode_clips_ladder_host(enc.h, dec.h, 70, enc._rungs(eight, int), 8, amd._p(h, amd._f32p), None, 100, amd._p(small.view(np.uint8), amd._u8p), 64,
                                                 amd._p(small, amd._i32p), None, small.ctypes.data, 1 << 30, amd._p(small, amd._i32p), None)
    assert rc == -1 and amd.lib().ulcx_last_error().decode() == "ulcx_encode_clips_ladder_host: " + why
    assert not small.any() and enc.last_rungs() == 3
    got = _call(codec).run()
    check_files(got, _refs(), "the call behind the refused ones")
    check_avg(got, bs, ch, "the call behind the refused ones")


def test_more_files_than_the_row_kernels_grid():
    bs, ch, streams, maxk = ct.GRID_GEOM
    amd = _amd()
    case = ct.grid_case(bs)
    refs = lt.refs(bs, ch, lt.GRID_RUNGS, case)
    enc = amd.BatchEncoder(streams, ch, bs, ct.RATE, maxk)
    dec = amd.BatchDecoder(8, ch, bs, maxk)
    try:
        got = LadderCall(enc, dec, bs, ch, lt.GRID_RUNGS, n=streams, streams=streams, case=case).run()
    finally:
        enc.close(); dec.close()
    F = 2 * streams
    f = np.arange(F)
    pick = (f // streams) * 7 + (f % streams) % 7          # file -> its reference among the 2 x 7
    flat = [r for g in refs for r in g]
    for name, have, want in (("d_indexBlocks", got.count, [r.nb for r in flat]), ("d_payloadBytes", got.nbytes, [r.payload.size for r in flat]),
                             ("d_maxBlock", got.maxb, [int(r.sizes.max()) if r.nb else 0 for r in flat])):
        bad = np.flatnonzero(have != np.array(want, np.int32)[pick])
        assert bad.size == 0, f"{name}: {bad.size} files differ from the oracle's, first file {bad[0]}: {have[bad[0]]}, last file {bad[-1]}"
    want = np.zeros((14, got.pstride), np.uint8)
    for j, r in enumerate(flat):
        want[j, :r.payload.size] = r.payload
    defined = np.arange(got.pstride)[None, :] < np.array([r.payload.size for r in flat])[:, None]
    bad = np.flatnonzero(((got.payload != want[pick]) & defined[pick]).any(axis=1))
    assert bad.size == 0, f"payload: {bad.size} files differ from the oracle's, first file {bad[0]}, last file {bad[-1]}"
    bad = np.flatnonzero(((got.payload != got.poison) & ~defined[pick]).any(axis=1))
    assert bad.size == 0, f"payload: {bad.size} files have bytes written behind their end, first file {bad[0]}"
    index = np.stack([r.index_row(got.istride) for r in flat])
    bad = np.flatnonzero((got.index.view(np.uint8).reshape(F, -1) != index[pick].view(np.uint8).reshape(F, -1)).any(axis=1))
    assert bad.size == 0, f"index: {bad.size} files differ from the oracle's walk, first file {bad[0]}, last file {bad[-1]}"
    check_avg(got, bs, ch, "grid")                          # no AUTO rung: not written
