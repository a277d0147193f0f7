"""Clip spectra on the GPU (include/ulc_amd.h section 3: ulcx_analyse_clips_*, ulcx_encode_clips_spectra_*): the encoder's own
MDCT coefficients of clips, channels-first, with each block's window code and complexity.  Every comparison of the planes is bit
for bit against the oracle (clip_spectra_testlib: oracle_encode_debug's coef, wc and cplx of the interleaved clip zero-padded to
the tool's block count; LR: numpy float32 m + s / m - s of those planes).  The encode form's corpus is compared array for array
with the plain clips call's on the same rows (which tests/test_gpu_clips.py holds to the oracle).
Shapes: tests/test_gpu_clips.py's - (BlockSize, nChan) = (256, 2), (512, 1), (256, 3); maxBlocksPerCall = 2, so a call is four
chunks; seven rows of 0, 1, BS - 1, BS, BS + 1, 3 * BS + 7 and 5 * BS + 3 samples on an object of 9 streams - with plane depths
8 (exact), 5 (cuts rows 5 and 6 inside a chunk) and 11 (three planes behind the last chunk).  All outputs sit on poisoned buffers
between guards.  tests/test_gpu_clip_spectra_paths.py runs the same call (SpecCall) on the encoder's fast paths and at scale."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import guarded_buffers as gb
import clips_testlib as ct
import clip_spectra_testlib as cs
from spectra_testlib import same_bits
from ulc_testlib import synth_pcm, oracle_encode_debug
from test_gpu_clips import Call, _amd, _dev

pytestmark = pytest.mark.gpu
N, B, MAXK = 7, 9, 2
FORMS = ("analyse", "encode")


class SpecCall(Call):
    """One ulcx_analyse_clips_dev(_pcm16) or ulcx_encode_clips_spectra_dev(_pcm16) call: test_gpu_clips.Call's rows and corpus
    buffers, and the three planes on a guarded arena of their own.  form "analyse" leaves the corpus buffers alone."""

    def __init__(self, enc, dec, bs, ch, n_blocks, form="encode", flags=0, null_wc=False, null_cplx=False, **kw):
        kw.setdefault("n", N)
        kw.setdefault("streams", B)
        super().__init__(enc, dec, bs, ch, **kw)
        G = min(kw["streams"], 8)
        self.form, self.n_blocks, self.flags, self.bs, self.ch = form, n_blocks, flags, bs, ch
        plane = lambda name: dict(name=name, nbytes=4 * self.n * n_blocks, align=4, role="out", guard=4 * G * n_blocks, row=4 * n_blocks)
        specs = [dict(name="d_coef", nbytes=4 * self.n * ch * n_blocks * bs, align=16, role="out", guard=4 * G * ch * n_blocks * bs, row=4 * bs,
                      rows_per_stream=ch * n_blocks)]
        specs += [] if null_wc else [plane("d_wc")]
        specs += [] if null_cplx else [plane("d_cplx")]
        self.t = gb.build(_dev(), specs)

    def run(self):
        import torch
        a, t = self.a, self.t
        opt = lambda arena, name: arena.ptr(name) if name in arena.regions else 0
        if self.form == "analyse":
            self.enc.analyse_clips_dev(self.n, a.ptr("d_pcm"), opt(a, "d_len"), self.T, self.n_blocks, t.ptr("d_coef"), opt(t, "d_wc"), opt(t, "d_cplx"),
                                       flags=self.flags, pcm16=self.args["pcm16"])
        else:
            self.enc.encode_clips_spectra_dev(self.dec, self.n, a.ptr("d_pcm"), opt(a, "d_len"), self.T, a.ptr("d_payload"), self.pstride, a.ptr("d_payloadBytes"),
                                              a.ptr("d_index"), self.istride, a.ptr("d_indexBlocks"), self.n_blocks, t.ptr("d_coef"), opt(t, "d_wc"), opt(t, "d_cplx"),
                                              flags=self.flags, d_max_block=a.ptr("d_maxBlock"), **self.args)
        torch.cuda.synchronize()
        a.check(); t.check()
        self.coef = t.fetch("d_coef", np.float32).reshape(self.n, self.ch, self.n_blocks, self.bs)
        self.wc = t.fetch("d_wc", np.int32).reshape(self.n, self.n_blocks) if "d_wc" in t.regions else None
        self.cplx = t.fetch("d_cplx", np.float32).reshape(self.n, self.n_blocks) if "d_cplx" in t.regions else None
        self.payload = a.fetch("d_payload").reshape(self.n, self.pstride)
        self.nbytes, self.maxb, self.count = a.fetch("d_payloadBytes", np.int32), a.fetch("d_maxBlock", np.int32), a.fetch("d_indexBlocks", np.int32)
        self.index = a.fetch("d_index", ct.INDEX_DTYPE).reshape(self.n, self.istride)
        if self.form == "analyse":                          # no corpus: those buffers keep their poison
            for name in ("d_payload", "d_payloadBytes", "d_maxBlock", "d_index", "d_indexBlocks"):
                r = a.regions[name]
                assert np.array_equal(a.fetch(name), gb.pattern(r.off, r.nbytes)), f"the analysis form wrote {name}"
        return self

    def check(self, refs, what):
        cs.check_planes(self.coef, self.wc, self.cplx, refs, self.n_blocks, bool(self.flags & cs.SPECTRA_LR), what)
        return self


def same_corpus(a, b, what):
    """Two clips calls' corpus outputs, array for array (of a payload the bytes that are defined)."""
    assert a.nbytes.tolist() == b.nbytes.tolist() and a.count.tolist() == b.count.tolist() and a.maxb.tolist() == b.maxb.tolist(), f"{what}: counts"
    assert a.index.tobytes() == b.index.tobytes(), f"{what}: index"
    for i in range(a.n):
        assert a.payload[i, :a.nbytes[i]].tobytes() == b.payload[i, :b.nbytes[i]].tobytes(), f"{what}: row {i}: payload bytes"


@pytest.fixture(scope="module", params=ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def codec(request):
    amd = _amd()
    bs, ch = request.param
    enc = amd.BatchEncoder(B, ch, bs, ct.RATE, MAXK)
    dec = amd.BatchDecoder(B, ch, bs, 12)
    yield bs, ch, enc, dec
    enc.close(); dec.close()


@pytest.mark.parametrize("pcm16", (False, True), ids=("float", "pcm16"))
@pytest.mark.parametrize("form", FORMS)
def test_planes_are_the_oracles_at_every_depth(codec, form, pcm16):
    bs, ch, enc, dec = codec
    refs = cs.specs(bs, ch)
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 6, 8]
    for depth in cs.DEPTHS:
        for flags in (0, cs.SPECTRA_LR):
            got = SpecCall(enc, dec, bs, ch, depth, form=form, flags=flags, pcm16=pcm16).run()
            got.check(refs, f"{form} {'pcm16' if pcm16 else 'float'} depth {depth} flags {flags}")
            assert not got.coef[0].any() and got.wc[0].tolist() == [0] * depth          # the empty row
            if depth > 8:
                assert not got.coef[:, :, 8:].view(np.uint32).any() and not got.wc[:, 8:].any() and not got.cplx[:, 8:].view(np.uint32).any()


@pytest.mark.parametrize("form", FORMS)
def test_wc_and_cplx_are_optional_one_at_a_time(codec, form):
    bs, ch, enc, dec = codec
    refs = cs.specs(bs, ch)
    a = SpecCall(enc, dec, bs, ch, 8, form=form, null_wc=True).run().check(refs, f"{form}, d_wc NULL")
    b = SpecCall(enc, dec, bs, ch, 8, form=form, null_cplx=True).run().check(refs, f"{form}, d_cplx NULL")
    assert a.wc is None and a.cplx is not None and b.cplx is None and b.wc is not None


@pytest.mark.parametrize("form", FORMS)
def test_null_len_takes_every_row_at_nsamples(codec, form):
    bs, ch, enc, dec = codec
    got = SpecCall(enc, dec, bs, ch, 8, form=form, null_len=True).run()
    full = [cs.SpecRef(bs, ch, ct.wave(bs, ch)[i]) for i in (0, 6)]
    cs.check_planes(got.coef[[0, 6]], got.wc[[0, 6]], got.cplx[[0, 6]], full, 8, False, f"{form}, d_len NULL, rows 0 and 6")
    assert (got.wc != 0).all()


def test_the_encode_forms_corpus_is_the_plain_calls(codec):
    bs, ch, enc, dec = codec
    refs, crefs = cs.specs(bs, ch), ct.refs(bs, ch)
    for kw, what in ((dict(), "VBR 50"), (dict(table=True), "per-row table"), (dict(pcm16=True), "pcm16")):
        plain = Call(enc, dec, bs, ch, n=N, streams=B, **kw).run()
        tap = SpecCall(enc, dec, bs, ch, 8, flags=cs.SPECTRA_LR if kw else 0, **kw).run().check(refs, f"encode form, {what}")
        same_corpus(tap, plain, what)
    assert plain.count.tolist() == [0, 3, 3, 3, 4, 6, 8]
    # capacities that truncate rows: the corpus is the plain call's, the spectra stay complete
    short = int(crefs[6].sizes[:3].sum()) - 1               # the payload's stride a byte short of row 6's third block
    for kw, what, counts in ((dict(pstride=short), "payloadStride a byte short of row 6's third block", None), (dict(istride=5), "indexStride 5", [0, 3, 3, 3, 4, 4, 4])):
        plain = Call(enc, dec, bs, ch, n=N, streams=B, **kw).run()
        tap = SpecCall(enc, dec, bs, ch, 8, **kw).run().check(refs, f"encode form, {what}")
        same_corpus(tap, plain, what)
        assert tap.count[6] < 8 and (tap.wc[6] != 0).all() and tap.coef[6, :, 7].any(), what
        assert counts is None or tap.count.tolist() == counts
    assert crefs[6].kept(short, 9) == 2 and tap.count[6] == 4


def test_streaming_state_and_the_objects_last_call(codec):
    bs, ch, enc, dec = codec
    import torch
    amd = _amd()
    enc.reset()
    pcm = np.stack([synth_pcm(40 + s, 4 * bs, ch, ct.RATE, transient=True, seed=3) for s in range(B)])
    refs = cs.specs(bs, ch)

    def stream2(part):                                      # ulcx_encode_dev of two blocks of every stream
        d_pcm = torch.from_numpy(np.ascontiguousarray(part)).to(_dev())
        d_out = torch.zeros((B, 2, enc.slot), dtype=torch.uint8, device=_dev())
        d_bits = torch.zeros((B, 2), dtype=torch.int32, device=_dev())
        enc.encode_dev(d_pcm.data_ptr(), 2, d_out.data_ptr(), d_bits.data_ptr(), mode=0, p0=50.0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_bits.cpu().numpy()
    try:
        SpecCall(enc, dec, bs, ch, 8, form="analyse").run().check(refs, "in front of the streaming calls")
        out1, bits1 = stream2(pcm[:, :2 * bs])
        SpecCall(enc, dec, bs, ch, 8, form="analyse").run().check(refs, "analysis form between streaming calls")
        assert enc.last_rungs() == 0
        with pytest.raises(amd.UlcError, match="analysis call"):
            enc.debug_fetch(K=2, parts=("coef",))
        a = SpecCall(enc, dec, bs, ch, 8, form="encode", table=True).run().check(refs, "encode form between streaming calls")
        assert enc.last_rungs() == 1
        enc.debug_fetch(K=2, parts=("nout",))              # as after the clips call: the taps answer
        out2, bits2 = stream2(pcm[:, 2 * bs:])
        b = SpecCall(enc, dec, bs, ch, 8, form="encode", table=True).run().check(refs, "the second encode form")
    finally:
        enc.reset()
    out, bits = np.concatenate([out1, out2], 1), np.concatenate([bits1, bits2], 1)
    for s in range(B):
        ref = oracle_encode_debug(pcm[s], bs, ct.RATE, 0, 50.0, slot=enc.slot)
        assert np.array_equal(bits[s], ref["bits"]), (s, bits[s], ref["bits"])
        for k in range(4):
            assert np.array_equal(out[s, k, :bits[s, k] // 8], ref["out"][k, :bits[s, k] // 8]), f"stream {s} block {k}: a clip-spectra call disturbed the stream"
    same_corpus(a, b, "the second encode form")


@pytest.mark.parametrize("lr", (False, True), ids=("ms", "lr"))
def test_pairing_with_the_decode_sides_spectra(codec, lr):
    """The encode form, then ulcx_decode_crops_spectra_dev of rows (file i, first 0) on its corpus: the same window codes on
    every block that has a coded partner, and the same blocks live."""
    import torch
    bs, ch, enc, dec = codec
    flags = cs.SPECTRA_LR if lr else 0
    got = SpecCall(enc, dec, bs, ch, 8, flags=flags).run().check(cs.specs(bs, ch), "pairing, the clean half")
    a, dev = got.a, _dev()
    d_file = torch.arange(N, dtype=torch.int32, device=dev)
    d_first = torch.zeros(N, dtype=torch.int32, device=dev)
    coef = torch.full((N, ch, 8, bs), float("nan"), dtype=torch.float32, device=dev)
    wc = torch.full((N, 8), -1, dtype=torch.int32, device=dev)
    bits = torch.full((N, 8), -1, dtype=torch.int32, device=dev)
    dec.decode_crops_spectra_dev(N, a.ptr("d_payload"), got.pstride, a.ptr("d_payloadBytes"), a.ptr("d_index"), got.istride, a.ptr("d_indexBlocks"), N,
                                 d_file.data_ptr(), d_first.data_ptr(), 0, 8, flags, coef.data_ptr(), wc.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    coef, wc, bits = coef.cpu().numpy(), wc.cpu().numpy(), bits.cpu().numpy()
    assert got.count.tolist() == [0, 3, 3, 3, 4, 6, 8]
    for i in range(N):
        m = int(got.count[i])
        assert np.array_equal(wc[i, :m], got.wc[i, :m]) and (wc[i, :m] != 0).all(), f"row {i}: window codes {wc[i].tolist()} vs the encoder's {got.wc[i].tolist()}"
        assert (bits[i, :m] > 0).all() and not bits[i, m:].any() and not wc[i, m:].any() and not got.wc[i, m:].any(), i
        assert not coef[i, :, m:].view(np.uint32).any() and not got.coef[i, :, m:].view(np.uint32).any(), i
        assert np.isfinite(coef[i]).all() and (m == 0 or coef[i, :, :m].any()), i


def test_host_forms(codec):
    bs, ch, enc, dec = codec
    refs = cs.specs(bs, ch)
    wave, lengths = ct.wave(bs, ch), ct.lengths(bs)
    for depth, lr in ((8, False), (5, True), (11, False)):
        coef, wc, cplx = enc.analyse_clips(wave, lengths, n_blocks=depth, flags=cs.SPECTRA_LR if lr else 0)
        cs.check_planes(coef, wc, cplx, refs, depth, lr, f"analysis host form, depth {depth}")
    coef, wc, cplx = enc.analyse_clips(wave, [0] * N, n_blocks=4)          # no row has a block: no chunk, the planes are zeros
    assert not coef.view(np.uint32).any() and not wc.any() and not cplx.view(np.uint32).any()
    plain = enc.encode_clips(dec, wave, lengths)
    r = enc.encode_clips_spectra(dec, wave, lengths, flags=cs.SPECTRA_LR)
    for x, y in zip(r[:5], plain):
        assert x.tobytes() == y.tobytes()
    cs.check_planes(r[5], r[6], r[7], refs, 8, True, "encode host form")
    amd = _amd()
    with pytest.raises(amd.UlcError, match="row 2 has -1 samples"):
        enc.analyse_clips(wave, [1, 2, -1, 4, 5, 6, 7])
    with pytest.raises(amd.UlcError, match="bad flags"):
        enc.analyse_clips(wave, lengths, flags=2)


def test_torch_front_end(codec):
    import torch
    import corpus
    bs, ch, enc, dec = codec
    refs = cs.specs(bs, ch)
    wave = torch.from_numpy(ct.wave(bs, ch)).to(_dev())
    coef, wc, cplx = corpus.clip_spectra(enc, wave, ct.lengths(bs), lr=True)
    torch.cuda.synchronize()
    cs.check_planes(coef.cpu().numpy(), wc.cpu().numpy(), cplx.cpu().numpy(), refs, 8, True, "corpus.clip_spectra")
    cor, coef, wc, cplx = corpus.CropCorpus.from_clips_spectra(enc, dec, wave, ct.lengths(bs), rate=(0, 50.0), n_blocks=5)
    torch.cuda.synchronize()
    cs.check_planes(coef.cpu().numpy(), wc.cpu().numpy(), cplx.cpu().numpy(), refs, 5, False, "CropCorpus.from_clips_spectra")
    assert cor.frozen and cor.d_index_blocks.cpu().tolist() == [r.nb for r in refs]
    coded, cwc, _ = cor.spectra(dec, list(range(N)), [0] * N, 5)
    torch.cuda.synchronize()
    assert np.array_equal(cwc.cpu().numpy(), wc.cpu().numpy())
