"""Clip spectra on the encoder's fast paths and at scale (include/ulc_amd.h section 3), beside tests/test_gpu_clip_spectra.py whose
shapes stay below every threshold of the launch sequence.  Every plane is compared bit for bit with the oracle's
(clip_spectra_testlib), the encode form's corpus array for array with the plain clips call's.

A. tests/test_gpu_clips_paths.py's geometries, (BlockSize, nChan, nStreams, maxBlocksPerCall) = (2048, 2, 70, 8), (4096, 2, 8, 8),
   (2048, 1, 8, 6), (16384, 1, 4, 2): clips of 23 blocks at the most, so the steady-state fast path of the transform, its general
   body, the pipelined front end and the transform of blocks above 8192 all feed the tap; rows end at every position of a chunk.
B. 16384 + 5 rows of (256, 1), 5 blocks deep, analysis form: more rows than the grid of the kernels that loop over rows.
tests/test_clip_spectra_capi.py checks on the CPU that the references hold decimated and un-decimated blocks behind the first chunk."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import clips_testlib as ct
import clip_spectra_testlib as cs
from test_gpu_clips import Call, _amd, _dev
from test_gpu_clip_spectra import SpecCall, same_corpus, FORMS

pytestmark = pytest.mark.gpu
G2048x2, G4096x2, G2048x1, G16384x1 = ct.PATH_GEOMS
_gid = lambda g: f"{g[0]}x{g[1]}"
_OBJECTS = {}
DEPTH = 23


def _codec(geom):
    """The geometry's encoder and decoder, made once for the module."""
    if geom not in _OBJECTS:
        amd = _amd()
        bs, ch, streams, maxk = geom
        _OBJECTS[geom] = (amd.BatchEncoder(streams, ch, bs, ct.RATE, maxk), amd.BatchDecoder(min(streams, 8), ch, bs, maxk))
    return _OBJECTS[geom]


@pytest.fixture(scope="module", autouse=True)
def _close_objects():
    yield
    for enc, dec in _OBJECTS.values():
        enc.close(); dec.close()
    _OBJECTS.clear()


def _rows(geom, rows=None):
    return list(ct.path_rows(*geom[:2])) if rows is None else list(rows)


def _call(geom, depth=DEPTH, rows=None, **kw):
    bs, ch, streams, _ = geom
    enc, dec = _codec(geom)
    rows = _rows(geom, rows)
    return SpecCall(enc, dec, bs, ch, depth, n=len(rows), streams=streams, case=ct.path_case(bs), rows=rows, **kw)


def _plain(geom, rows=None, **kw):
    bs, ch, streams, _ = geom
    enc, dec = _codec(geom)
    rows = _rows(geom, rows)
    return Call(enc, dec, bs, ch, n=len(rows), streams=streams, case=ct.path_case(bs), rows=rows, **kw)


def _specs(geom, rows=None):
    bs, ch = geom[:2]
    return cs.specs(bs, ch, case=ct.path_case(bs), rows=_rows(geom, rows))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", ct.PATH_GEOMS, ids=_gid)
def test_planes_over_pipelined_chunks_are_the_oracles(geom, form):
    refs = _specs(geom)
    assert [r.nb for r in refs] == [ct.PATH_BLOCKS[i] for i in _rows(geom)]
    got = _call(geom, form=form).run().check(refs, f"{form} at {_gid(geom)}, chunks of {geom[3]}")
    if form == "encode":
        same_corpus(got, _plain(geom).run(), f"the encode form's corpus at {_gid(geom)}")
        assert got.count.tolist() == [r.nb for r in refs]


@pytest.mark.parametrize("form", FORMS)
def test_pcm16_over_pipelined_chunks(form):
    """PCM16 input takes the transform's fast path from the third block on; two planes behind the last chunk."""
    got = _call(G2048x2, depth=DEPTH + 2, form=form, pcm16=True).run().check(_specs(G2048x2), f"{form} pcm16 at 2048x2")
    if form == "encode":
        same_corpus(got, _plain(G2048x2, pcm16=True).run(), "the encode form's corpus, pcm16 at 2048x2")


@pytest.mark.parametrize("geom", (G2048x2, G4096x2), ids=_gid)
def test_lr_over_pipelined_chunks_cut_inside_the_last_chunk(geom):
    """Planes of 20 blocks: the chunk of blocks 16 .. 22 is cut for the rows of 23 blocks."""
    _call(geom, depth=20, form="analyse", flags=cs.SPECTRA_LR).run().check(_specs(geom), f"analysis LR at {_gid(geom)}, 20 blocks deep")
    _call(geom, depth=20, form="encode", flags=cs.SPECTRA_LR, table=True).run().check(_specs(geom), f"encode LR under a table at {_gid(geom)}, 20 blocks deep")


@pytest.mark.parametrize("form", FORMS)
def test_rows_across_a_stream_group(form):
    """70 rows on the object of 70 streams, row i = pair i % 7: the window-control kernels' second stream group holds six rows."""
    rows = [i % 7 for i in range(70)]
    got = _call(G2048x2, rows=rows, form=form).run().check(_specs(G2048x2, rows), f"{form}, 70 rows on 70 streams")
    if form == "encode":
        assert got.count.tolist() == [ct.PATH_BLOCKS[i] for i in rows]


def test_more_rows_than_the_row_kernels_grid():
    """The analysis form on 16389 rows of 256 x 1, planes 5 blocks deep, on pre-poisoned tensors."""
    import torch
    bs, ch, streams, maxk = ct.GRID_GEOM
    amd = _amd()
    case = ct.grid_case(bs)
    refs = cs.specs(bs, ch, case=case)
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 4, 5]
    pair = np.arange(streams) % 7
    dev = _dev()
    wave = torch.from_numpy(ct.wave(bs, ch, case.T)[pair]).to(dev)
    d_len = torch.from_numpy(np.array(case.lengths, np.int32)[pair]).to(dev)
    coef = torch.full((streams, ch, 5, bs), float("nan"), dtype=torch.float32, device=dev)
    wc = torch.full((streams, 5), -1, dtype=torch.int32, device=dev)
    cplx = torch.full((streams, 5), float("nan"), dtype=torch.float32, device=dev)
    enc = amd.BatchEncoder(streams, ch, bs, ct.RATE, maxk)
    try:
        enc.analyse_clips_dev(streams, wave.data_ptr(), d_len.data_ptr(), case.T, 5, coef.data_ptr(), wc.data_ptr(), cplx.data_ptr())
        torch.cuda.synchronize()
    finally:
        enc.close()
    wcoef, wwc, wcplx = cs.expected(refs, 5)
    for name, have, want in (("d_coef", coef.cpu().numpy().view(np.uint32).reshape(streams, -1), wcoef.view(np.uint32).reshape(7, -1)),
                             ("d_wc", wc.cpu().numpy(), wwc), ("d_cplx", cplx.cpu().numpy().view(np.uint32), wcplx.view(np.uint32))):
        bad = np.flatnonzero((have != want[pair]).any(axis=1))
        assert bad.size == 0, f"{name}: {bad.size} rows differ from the oracle's, first row {bad[0]} (pair {bad[0] % 7}), last row {bad[-1]}"
