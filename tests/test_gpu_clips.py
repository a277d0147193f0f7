"""Clips on the GPU (include/ulc_amd.h section 3: ulcx_encode_clips_*, ulcx_corpus_ragged_*): rows are whole clips in samples,
channels-first, each at its own length and encoded from a fresh state; the output is a resident corpus.  Every comparison is
byte for byte against the oracle (clips_testlib: oracle_encode_debug of the interleaved clip zero-padded to the tool's block
count; the index from the oracle decoder's walk of that payload) - never against this library's own plain encode call.
Shapes: (BlockSize, nChan) = (256, 2), (512, 1), (256, 3); maxBlocksPerCall = 2, so a call is four chunks and rows end in the
middle of one; nSamples = 5 * BS + 3; seven rows of 0, 1, BS - 1, BS, BS + 1, 3 * BS + 7 and nSamples samples.  All outputs sit
on poisoned buffers between guards (tests/guarded_buffers.py).  tests/test_gpu_clips_paths.py runs the same call (Call, _check_rows)
at the shapes where the launch sequence pipelines its chunks, and at scale."""
import numpy as np
import pytest

from ulc_testlib import to_pcm16
from gpu_testlib import amd as _amd, dev as _dev
import guarded_buffers as gb
import clips_testlib as ct
from ulc_testlib import synth_pcm, oracle_encode_debug

pytestmark = pytest.mark.gpu
N, B, MAXK = 7, 8, 2


class Call:
    """One ulcx_encode_clips_dev(_pcm16) call on a guarded arena -> the outputs as numpy.  n rows on an object of `streams`
    streams; case: nSamples and the lengths of the seven (clip, length) pairs (clips_testlib.Case; default: this file's);
    rows: the pair of every row (default: row i is pair i % 7).  The call's chunks are the encoder's maxBlocksPerCall."""

    def __init__(self, enc, dec, bs, ch, pstride=None, istride=None, table=False, pcm16=False, null_len=False, n=N, streams=B, case=None, rows=None):
        case = case or ct.short_case(bs)
        rows = [i % 7 for i in range(n)] if rows is None else list(rows)
        assert len(rows) == n <= streams
        T, nb = case.T, ct.clip_blocks(bs, case.T)
        G = min(streams, 8)                                 # rows of a guard (the guards of a large object: as those of eight streams)
        self.n, self.T, self.rows, self.case = n, T, rows, case
        self.pstride = pstride or enc.slot * nb
        self.istride = istride or nb + 1
        esz = 2 if pcm16 else 4
        word = lambda name, k, role: dict(name=name, nbytes=4 * k, align=4, role=role, guard=4 * G, row=4)
        specs = [dict(name="d_pcm", nbytes=n * ch * T * esz, align=esz, role="in", guard=G * ch * T * esz, row=T * esz, rows_per_stream=ch)]
        if not null_len:
            specs.append(word("d_len", n, "in"))
        if table:
            specs.append(dict(name="d_rate", nbytes=8 * n, align=8, role="in", guard=8 * G, row=8))
        specs += [dict(name="d_payload", nbytes=n * self.pstride, align=1, role="out", guard=G * self.pstride, row=self.pstride),
                  word("d_payloadBytes", n, "out"), word("d_maxBlock", n, "out"),
                  dict(name="d_index", nbytes=8 * n * self.istride, align=4, role="out", guard=8 * G * self.istride, row=8, rows_per_stream=self.istride),
                  word("d_indexBlocks", n, "out")]
        a = self.a = gb.build(_dev(), specs)
        w = ct.wave(bs, ch, T)[rows]
        a.load("d_pcm", to_pcm16(w) if pcm16 else w)
        if not null_len:
            a.load("d_len", np.array(case.lengths, np.int32)[rows])
        if table:
            a.load("d_rate", np.array(ct.TABLE, np.float32)[rows])
        self.args = dict(pcm16=pcm16, d_rates=a.ptr("d_rate") if table else 0, mode=0, p0=50.0)
        self.enc, self.dec = enc, dec

    def run(self):
        import torch
        a = self.a
        self.enc.encode_clips_dev(self.dec, self.n, a.ptr("d_pcm"), a.ptr("d_len") if "d_len" in a.regions else 0, self.T, a.ptr("d_payload"), self.pstride,
                                  a.ptr("d_payloadBytes"), a.ptr("d_index"), self.istride, a.ptr("d_indexBlocks"), d_max_block=a.ptr("d_maxBlock"), **self.args)
        torch.cuda.synchronize()
        a.check()
        self.payload = a.fetch("d_payload").reshape(self.n, self.pstride)
        self.nbytes, self.maxb, self.count = a.fetch("d_payloadBytes", np.int32), a.fetch("d_maxBlock", np.int32), a.fetch("d_indexBlocks", np.int32)
        self.index = a.fetch("d_index", ct.INDEX_DTYPE).reshape(self.n, self.istride)
        return self


def _check_rows(got, refs, what, pstride=None, istride=None):
    """Every row against the oracle: the leading blocks the capacities keep (all of them by default)."""
    for i, r in enumerate(refs[:got.n]):
        m = r.kept(pstride or got.pstride, istride or got.istride)
        nbytes = int(r.sizes[:m].sum())
        where = f"{what}: row {i} ({r.L} samples, {r.nb} blocks, {m} kept)"
        assert got.count[i] == m, f"{where}: d_indexBlocks {got.count[i]}"
        assert got.nbytes[i] == nbytes, f"{where}: d_payloadBytes {got.nbytes[i]} vs the oracle's {nbytes}"
        assert got.maxb[i] == (int(r.sizes[:m].max()) if m else 0), f"{where}: d_maxBlock {got.maxb[i]}"
        if not np.array_equal(got.payload[i, :nbytes], r.payload[:nbytes]):
            bad = np.flatnonzero(got.payload[i, :nbytes] != r.payload[:nbytes])
            edges = np.concatenate([[0], np.cumsum(r.sizes)])
            raise AssertionError(f"{where}: {bad.size} of {nbytes} payload bytes differ from the oracle's, first at byte {bad[0]} "
                                 f"(block {int(np.searchsorted(edges, bad[0], 'right')) - 1}), last at {bad[-1]}")
        want = r.index_row(got.istride, m)
        assert got.index[i].tobytes() == want.tobytes(), f"{where}: index {got.index[i][:m + 2]} vs the oracle's walk {want[:m + 2]}"


@pytest.fixture(scope="module", params=ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def codec(request):
    amd = _amd()
    bs, ch = request.param
    enc = amd.BatchEncoder(B, ch, bs, ct.RATE, MAXK)
    dec = amd.BatchDecoder(B, ch, bs, amd.crop_blocks(bs, ct.n_samples(bs)) + 1)
    yield bs, ch, enc, dec
    enc.close(); dec.close()


def test_scalar_vbr_rows_are_the_oracles_files(codec):
    bs, ch, enc, dec = codec
    refs = ct.refs(bs, ch)
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 6, 8]
    got = Call(enc, dec, bs, ch).run()
    _check_rows(got, refs, "VBR 50")
    assert got.count.tolist() == [0, 3, 3, 3, 4, 6, 8] and got.nbytes[0] == 0
    assert got.index[0].tobytes() == _amd().new_index(1, got.istride)[0].tobytes()              # the empty row: the open index row
    full = Call(enc, dec, bs, ch, null_len=True).run()                                          # NULL d_len: every row nSamples long
    for i in range(N):
        r = ct.ClipRef(bs, ch, ct.wave(bs, ch)[i], ct.SCALAR) if i in (0, 6) else None          # (rows 0 and 6 checked: the oracle run is the cost)
        if r is not None:
            assert full.count[i] == r.nb and full.nbytes[i] == r.payload.size and np.array_equal(full.payload[i, :r.payload.size], r.payload), i
    assert got.payload[6, :got.nbytes[6]].tobytes() == full.payload[6, :full.nbytes[6]].tobytes()


def test_a_table_mixes_vbr_cbr_and_abr_rows(codec):
    bs, ch, enc, dec = codec
    got = Call(enc, dec, bs, ch, table=True).run()
    _check_rows(got, ct.refs(bs, ch, table=True), "per-row table")


def test_pcm16_equals_the_float_call_on_converted_input(codec):
    bs, ch, enc, dec = codec
    f = Call(enc, dec, bs, ch).run()
    h = Call(enc, dec, bs, ch, pcm16=True).run()
    _check_rows(h, ct.refs(bs, ch), "pcm16")
    for i in range(N):
        assert h.nbytes[i] == f.nbytes[i] and h.payload[i, :h.nbytes[i]].tobytes() == f.payload[i, :f.nbytes[i]].tobytes(), i
    assert h.index.tobytes() == f.index.tobytes() and h.count.tolist() == f.count.tolist() and h.maxb.tolist() == f.maxb.tolist()


def test_capacity_keeps_leading_whole_blocks(codec):
    bs, ch, enc, dec = codec
    refs = ct.refs(bs, ch)
    whole = Call(enc, dec, bs, ch).run()
    # the payload's stride a byte short of row 6's third block
    short = int(refs[6].sizes[:3].sum()) - 1
    got = Call(enc, dec, bs, ch, pstride=short).run()
    assert refs[6].kept(short, got.istride) == 2 and got.count[6] == 2 and got.nbytes[6] == int(refs[6].sizes[:2].sum())
    _check_rows(got, refs, "payloadStride a byte short of row 6's third block")
    fit = [i for i in range(N) if refs[i].kept(short, got.istride) == refs[i].nb]
    assert len(fit) >= 2
    for i in fit:                                           # the rows that fit are what they are without the limit
        assert got.nbytes[i] == whole.nbytes[i] and got.payload[i, :got.nbytes[i]].tobytes() == whole.payload[i, :whole.nbytes[i]].tobytes(), i
    # indexStride - 1 = 4: below the 6 and 8 blocks of rows 5 and 6, exactly row 4's
    got = Call(enc, dec, bs, ch, istride=5).run()
    assert got.count.tolist() == [0, 3, 3, 3, 4, 4, 4]
    _check_rows(got, refs, "indexStride 5")
    for i in range(5):
        assert got.payload[i, :got.nbytes[i]].tobytes() == whole.payload[i, :whole.nbytes[i]].tobytes(), i
    for i in (5, 6):
        assert got.nbytes[i] == int(refs[i].sizes[:4].sum()) and got.index[i]["ByteOffs"][4] == got.nbytes[i]


def test_streaming_state_is_untouched_and_a_second_call_repeats_the_first(codec):
    bs, ch, enc, dec = codec
    enc.reset()
    pcm = np.stack([synth_pcm(40 + s, 4 * bs, ch, ct.RATE, transient=True, seed=3) for s in range(B)])
    import torch

    def stream2(part):                                      # ulcx_encode_dev of two blocks of every stream
        d_pcm = torch.from_numpy(np.ascontiguousarray(part)).to(_dev())
        d_out = torch.zeros((B, 2, enc.slot), dtype=torch.uint8, device=_dev())
        d_bits = torch.zeros((B, 2), dtype=torch.int32, device=_dev())
        enc.encode_dev(d_pcm.data_ptr(), 2, d_out.data_ptr(), d_bits.data_ptr(), mode=0, p0=50.0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_bits.cpu().numpy()
    out1, bits1 = stream2(pcm[:, :2 * bs])
    a = Call(enc, dec, bs, ch, table=True).run()
    out2, bits2 = stream2(pcm[:, 2 * bs:])
    b = Call(enc, dec, bs, ch, table=True).run()
    out, bits = np.concatenate([out1, out2], 1), np.concatenate([bits1, bits2], 1)
    for s in range(B):
        ref = oracle_encode_debug(pcm[s], bs, ct.RATE, 0, 50.0, slot=enc.slot)
        assert np.array_equal(bits[s], ref["bits"]), (s, bits[s], ref["bits"])
        for k in range(4):
            assert np.array_equal(out[s, k, :bits[s, k] // 8], ref["out"][k, :bits[s, k] // 8]), f"stream {s} block {k}: the clips call disturbed the stream"
    _check_rows(a, ct.refs(bs, ch, table=True), "between streaming calls")
    assert a.nbytes.tolist() == b.nbytes.tolist() and a.index.tobytes() == b.index.tobytes() and a.count.tolist() == b.count.tolist()
    for i in range(N):
        assert a.payload[i, :a.nbytes[i]].tobytes() == b.payload[i, :b.nbytes[i]].tobytes(), i
    enc.reset()


def test_host_form(codec):
    bs, ch, enc, dec = codec
    payload, nbytes, maxb, index, count = enc.encode_clips(dec, ct.wave(bs, ch), ct.lengths(bs))

    class Got:
        pass
    g = Got()
    g.n, g.payload, g.nbytes, g.maxb, g.index, g.count = N, payload, nbytes, maxb, index, count
    g.pstride, g.istride = payload.shape[1], index.shape[1]
    _check_rows(g, ct.refs(bs, ch), "host form")
    amd = _amd()
    with pytest.raises(amd.UlcError, match="row 2 has -1 samples"):
        enc.encode_clips(dec, ct.wave(bs, ch), [1, 2, -1, 4, 5, 6, 7])
    with pytest.raises(amd.UlcError, match="invalid entry for row 3"):
        enc.encode_clips(dec, ct.wave(bs, ch), ct.lengths(bs), rates=[(-50.0, 0.0)] * 3 + [(0.0, 0.0)] + [(64.0, 0.0)] * 3)


def _expected_crop(r, start, T):
    """[ch][T]: the oracle's decode of the clip's blocks from sample `start`, zeros behind the file's end."""
    out = np.zeros((r.ch, T), np.float32)
    if r.nb and start // r.bs <= r.nb:
        stream = r.decoded().T
        end = min(start + T, r.nb * r.bs)
        if end > start:
            out[:, :end - start] = stream[:, start:end]
    return out


@pytest.mark.parametrize("layout", ("strided", "ragged"))
def test_round_trip_from_clips_then_sample_crops(codec, layout):
    import torch
    import corpus
    bs, ch, enc, dec = codec
    T = ct.n_samples(bs)
    wave = torch.from_numpy(ct.wave(bs, ch)).to(_dev())
    cor = corpus.CropCorpus.from_clips(enc, dec, wave, ct.lengths(bs), rate=(0, 50.0), layout=layout)
    assert cor.frozen and len(cor) == N
    pcm, _ = cor.sample_crops(dec, list(range(N)), [2 * bs] * N, T)
    torch.cuda.synchronize()
    pcm = pcm.cpu().numpy()
    refs = ct.refs(bs, ch)
    for i, r in enumerate(refs):
        want = _expected_crop(r, 2 * bs, T)
        assert pcm[i].tobytes() == want.tobytes(), f"{layout}: row {i}: {(pcm[i].view(np.uint32) != want.view(np.uint32)).sum()} samples differ from the oracle's decode"
    assert cor.d_index_blocks.cpu().tolist() == [r.nb for r in refs]
    assert (pcm[6] != 0).any() and (pcm[0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# strided corpus -> ragged corpus
# ---------------------------------------------------------------------------------------------------------------------
ROWS5 = (1, 0, 5, 4, 6)                                     # a 5-file corpus of the rows above, the empty one among them


def _strided5(bs, ch):
    refs = [ct.refs(bs, ch)[i] for i in ROWS5]
    stride = max(r.payload.size for r in refs) + 13          # odd: the files start at every alignment
    istride = 9
    pay = np.full((5, stride), 0xA5, np.uint8)
    nbytes = np.array([r.payload.size for r in refs], np.int32)
    index = np.zeros((5, istride), ct.INDEX_DTYPE)
    for f, r in enumerate(refs):
        pay[f, :r.payload.size] = r.payload
        index[f] = r.index_row(istride)
    return refs, pay, nbytes, index, np.array([r.nb for r in refs], np.int32)


def _ragged_call(pay, nbytes, index, blocks, pcap, icap):
    import torch
    amd = _amd()
    F, stride = pay.shape
    istride = index.shape[1]
    word = lambda name, k, role, sz=4: dict(name=name, nbytes=sz * k, align=sz, role=role, guard=sz * 8, row=sz)
    specs = [dict(name="d_payload", nbytes=F * stride, align=1, role="in", guard=F * stride, row=stride), word("d_payloadBytes", F, "in"),
             dict(name="d_index", nbytes=8 * F * istride, align=4, role="in", guard=8 * F * istride, row=8, rows_per_stream=istride), word("d_indexBlocks", F, "in"),
             dict(name="d_outPayload", nbytes=max(1, pcap), align=1, role="out", guard=F * stride, row=max(1, pcap)),
             word("d_payloadOffs", F + 1, "out", 8), dict(name="d_outIndex", nbytes=8 * max(1, icap), align=4, role="out", guard=8 * F * istride, row=8),
             word("d_indexOffs", F + 1, "out", 8), word("d_outIndexBlocks", F, "out"), word("d_need", 2, "out", 8)]
    a = gb.build(_dev(), specs)
    a.load("d_payload", pay); a.load("d_payloadBytes", nbytes); a.load("d_index", index); a.load("d_indexBlocks", blocks)
    amd.corpus_ragged_dev(F, a.ptr("d_payload"), stride, a.ptr("d_payloadBytes"), a.ptr("d_index"), istride, a.ptr("d_indexBlocks"), a.ptr("d_outPayload"), pcap,
                          a.ptr("d_payloadOffs"), a.ptr("d_outIndex"), icap, a.ptr("d_indexOffs"), a.ptr("d_outIndexBlocks"), a.ptr("d_need"))
    torch.cuda.synchronize()
    a.check()
    return a


def _check_ragged(a, pay, nbytes, index, blocks, pcap, icap, what):
    F, stride = pay.shape
    istride = index.shape[1]
    poffs, ioffs, oblocks, need = ct.ragged_plan(nbytes, stride, blocks, istride, pcap, icap)
    assert a.fetch("d_payloadOffs", np.int64).tolist() == poffs.tolist(), what
    assert a.fetch("d_indexOffs", np.int64).tolist() == ioffs.tolist(), what
    assert a.fetch("d_outIndexBlocks", np.int32).tolist() == oblocks.tolist(), what
    assert a.fetch("d_need", np.int64).tolist() == need.tolist(), what
    op, oi = a.fetch("d_outPayload"), a.fetch("d_outIndex", ct.INDEX_DTYPE)
    for f in range(F):
        nb, ne = int(poffs[f + 1] - poffs[f]), int(ioffs[f + 1] - ioffs[f])
        assert op[poffs[f]:poffs[f + 1]].tobytes() == pay[f, :nb].tobytes(), f"{what}: file {f}: payload bytes"
        assert oi[ioffs[f]:ioffs[f + 1]].tobytes() == index[f, :ne].tobytes(), f"{what}: file {f}: index row"
    return poffs, ioffs, oblocks, need


@pytest.mark.parametrize("geom", ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_strided_corpus_to_ragged_and_its_crops(geom):
    import torch
    amd = _amd()
    bs, ch = geom
    refs, pay, nbytes, index, blocks = _strided5(bs, ch)
    need = ct.ragged_plan(nbytes, pay.shape[1], blocks, index.shape[1], 1 << 40, 1 << 40)[3]
    pcap, icap = int(need[0]), int(need[1])
    a = _ragged_call(pay, nbytes, index, blocks, pcap, icap)
    poffs, ioffs, oblocks, _ = _check_ragged(a, pay, nbytes, index, blocks, pcap, icap, "whole corpus")
    assert poffs[-1] == pcap and ioffs[-1] == icap and oblocks.tolist() == blocks.tolist()
    # the result is what the ragged sample-crop call reads
    T = ct.n_samples(bs)
    dec = amd.BatchDecoder(B, ch, bs, amd.crop_blocks(bs, T) + 1)
    files, start = [0, 1, 2, 3, 4, 4], [2 * bs, 0, bs + 5, 2 * bs - 1, 2 * bs, 0]
    d_file = torch.tensor(files, dtype=torch.int32, device=_dev())
    d_start = torch.tensor(start, dtype=torch.int64, device=_dev())
    pcm = torch.full((len(files), ch, T), 7.0, dtype=torch.float32, device=_dev())
    bits = torch.full((len(files), amd.crop_blocks(bs, T)), 7, dtype=torch.int32, device=_dev())
    dec.decode_crops_samples_ragged_dev(5, a.ptr("d_outPayload"), pcap, a.ptr("d_payloadOffs"), a.ptr("d_outIndex"), icap, a.ptr("d_indexOffs"),
                                        a.ptr("d_outIndexBlocks"), len(files), d_file.data_ptr(), d_start.data_ptr(), 0, T, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    got = pcm.cpu().numpy()
    for i, (f, s) in enumerate(zip(files, start)):
        want = _expected_crop(refs[f], s, T)
        assert got[i].tobytes() == want.tobytes(), f"row {i} (file {f} from sample {s}): differs from the oracle's decode"
    dec.close()
    # a payload capacity that cuts before file 3: files 3 and 4 come out empty, the need is the whole corpus's
    cut = int(poffs[3]) + int(nbytes[3]) - 1
    a = _ragged_call(pay, nbytes, index, blocks, cut, icap)
    p2, i2, b2, n2 = _check_ragged(a, pay, nbytes, index, blocks, cut, icap, "payloadCap cuts before file 3")
    assert b2.tolist()[3:] == [0, 0] and p2[3] == p2[4] == p2[5] and i2[3] == i2[4] == i2[5] and n2.tolist() == [pcap, icap]
    # the host form, on the same corpus
    r = amd.corpus_ragged(pay, nbytes, index, blocks)
    assert r["payload_offs"].tolist() == poffs.tolist() and r["index_offs"].tolist() == ioffs.tolist() and r["need"].tolist() == [pcap, icap]
    assert r["payload"][:pcap].tobytes() == b"".join(x.payload.tobytes() for x in refs)
