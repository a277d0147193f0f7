"""Clips under a rate ladder on the GPU (include/ulc_amd.h section 3: ulcx_encode_clips_ladder_*, ULCX_RUNG_AUTO): one call, one
corpus of nRungs * n files, file r * n + i = clip i under rung r.  Every file is compared byte for byte and entry for entry with
the oracle's (clips_ladder_testlib: clips_testlib.ClipRef of the clip under the rung's setting for that row; an AUTO rung's
setting holds the average formed in Python from the oracle's complexities) - never with this library's own plain clips call.
Shapes below every threshold of the launch sequence, as tests/test_gpu_clips.py: (BlockSize, nChan) = (256, 2), (512, 1), (256, 3),
seven rows on an object of eight streams, maxBlocksPerCall = 2 (four chunks; rows end in the middle of one).  All outputs sit on
poisoned buffers between guards.  tests/test_gpu_clips_ladder_paths.py runs the same call (LadderCall, check_files) on the
pipelined front end and at scale; tests/test_clips_ladder_capi.py checks on the CPU what these tests lean on."""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import clips_testlib as ct
import clips_ladder_testlib as lt
from ulc_testlib import synth_pcm, oracle_encode_debug
from clips_ladder_testlib import LadderCall, check_files, check_avg, _amd, _dev

pytestmark = pytest.mark.gpu
N, B, MAXK = 7, 8, 2


@pytest.fixture(scope="module", params=ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def codec(request):
    amd = _amd()
    bs, ch = request.param
    enc = amd.BatchEncoder(B, ch, bs, ct.RATE, MAXK)
    dec = amd.BatchDecoder(B, ch, bs, amd.crop_blocks(bs, ct.n_samples(bs)) + 1)
    yield bs, ch, enc, dec
    enc.close(); dec.close()


@pytest.mark.parametrize("pcm16", (False, True), ids=("float", "pcm16"))
def test_five_rungs_are_the_oracles_files(codec, pcm16):
    bs, ch, enc, dec = codec
    refs = lt.refs(bs, ch, lt.FIVE)
    got = LadderCall(enc, dec, bs, ch, lt.FIVE, pcm16=pcm16).run()
    check_files(got, refs, "VBR 50 | TABLE | CBR 64 | AUTO 96 | AUTO on TABLE")
    check_avg(got, bs, ch, "five rungs")
    assert got.count.reshape(5, N).tolist() == [[0, 3, 3, 3, 4, 6, 8]] * 5 and got.avg[0] == 0
    assert got.index[0].tobytes() == _amd().new_index(1, got.istride)[0].tobytes()              # an empty row: the open index row
    assert enc.last_rungs() == 5


def test_eight_rungs(codec):
    bs, ch, enc, dec = codec
    got = LadderCall(enc, dec, bs, ch, lt.EIGHT).run()
    check_files(got, lt.refs(bs, ch, lt.EIGHT), "eight rungs")
    check_avg(got, bs, ch, "eight rungs")


def test_one_rung_without_auto_and_the_optional_pointers(codec):
    bs, ch, enc, dec = codec
    got = LadderCall(enc, dec, bs, ch, (lt.TABLE,)).run()
    check_files(got, lt.refs(bs, ch, (lt.TABLE,)), "one table rung")
    check_avg(got, bs, ch, "one table rung")                # not written
    # d_maxBlock = NULL, d_avg = NULL - with an AUTO rung
    got = LadderCall(enc, dec, bs, ch, (lt.VBR50, lt.AUTO96), null_opt=True).run()
    check_files(got, lt.refs(bs, ch, (lt.VBR50, lt.AUTO96)), "no d_maxBlock, no d_avg")


def test_null_len_reads_every_row_in_full(codec):
    bs, ch, enc, dec = codec
    rungs = (lt.VBR50, lt.AUTO96)
    got = LadderCall(enc, dec, bs, ch, rungs, null_len=True).run()
    w = ct.wave(bs, ch)
    nb = ct.clip_blocks(bs, w.shape[2])
    assert nb == 8 and got.count.tolist() == [8] * (2 * N)  # every row is nSamples long, its own length or not
    avgs = []
    for i in range(N):                                      # every row's average: one oracle run of eight blocks each
        pcm = np.concatenate([w[i].T, np.zeros((nb * bs - w.shape[2], ch), np.float32)])
        avgs.append(lt.avg_of(oracle_encode_debug(pcm, bs, ct.RATE, 0, 50.0)["cplx"]))
    assert got.avg.tobytes() == np.array(avgs, np.float32).tobytes(), (got.avg, avgs)
    for i in (0, 6):                                        # (files of rows 0 and 6: the oracle runs are the cost; row 6 is the short case's too)
        for r, st in enumerate(((-50.0, 0.0), (96.0, float(avgs[i])))):
            ref = ct.ClipRef(bs, ch, w[i], st)
            f = r * N + i
            assert got.nbytes[f] == ref.payload.size and np.array_equal(got.payload[f, :ref.payload.size], ref.payload), (i, r)
            assert got.index[f].tobytes() == ref.index_row(got.istride).tobytes(), (i, r)


def test_capacity_is_per_file(codec):
    bs, ch, enc, dec = codec
    refs = lt.refs(bs, ch, lt.FIVE)
    hi, lo, m, stride = lt.ladder_cut(bs, ch)
    got = LadderCall(enc, dec, bs, ch, lt.FIVE, pstride=stride).run()
    assert got.count[hi * N + 6] == m < 8 == got.count[lo * N + 6]      # the high-rate rung stops in a later chunk, the low-rate one is whole
    check_files(got, refs, f"payloadStride {stride}: a byte short of block {m} of row 6 under rung {hi}")
    check_avg(got, bs, ch, "payload capacity")              # all of the clip's blocks count, whatever the capacity keeps
    got = LadderCall(enc, dec, bs, ch, lt.FIVE, istride=5).run()
    assert got.count.reshape(5, N).tolist() == [[0, 3, 3, 3, 4, 4, 4]] * 5
    check_files(got, refs, "indexStride 5")
    check_avg(got, bs, ch, "index capacity")
    for r in range(5):
        for i in (5, 6):
            f = r * N + i
            assert got.index[f]["ByteOffs"][4] == got.nbytes[f] == int(refs[r][i].sizes[:4].sum())


def _expected_crop(r, start, T):
    """[ch][T]: the oracle's decode of the file's blocks from sample `start`, zeros behind the file's end."""
    out = np.zeros((r.ch, T), np.float32)
    if r.nb and start // r.bs <= r.nb:
        stream = r.decoded().T
        end = min(start + T, r.nb * r.bs)
        if end > start:
            out[:, :end - start] = stream[:, start:end]
    return out


def test_the_corpus_is_what_the_sample_crop_call_reads(codec):
    import torch
    bs, ch, enc, dec = codec
    amd = _amd()
    rungs = (lt.VBR50, lt.AUTO96, lt.TABLE)
    refs = lt.refs(bs, ch, rungs)
    c = LadderCall(enc, dec, bs, ch, rungs).run()
    T = ct.n_samples(bs)
    files = [r * N + i for r, i in ((0, 6), (1, 6), (2, 6), (1, 5), (2, 1), (1, 0), (0, 4), (2, 4))]
    start = [2 * bs, 2 * bs, bs + 5, 0, 0, 0, 2 * bs - 1, bs]
    d_file = torch.tensor(files, dtype=torch.int32, device=_dev())
    d_start = torch.tensor(start, dtype=torch.int64, device=_dev())
    pcm = torch.full((len(files), ch, T), 7.0, dtype=torch.float32, device=_dev())
    bits = torch.full((len(files), amd.crop_blocks(bs, T)), 7, dtype=torch.int32, device=_dev())
    a = c.a
    dec.decode_crops_samples_dev(c.F, a.ptr("d_payload"), c.pstride, a.ptr("d_payloadBytes"), a.ptr("d_index"), c.istride, a.ptr("d_indexBlocks"),
                                 len(files), d_file.data_ptr(), d_start.data_ptr(), 0, T, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    got = pcm.cpu().numpy()
    for j, (f, s) in enumerate(zip(files, start)):
        want = _expected_crop(refs[f // N][f % N], s, T)
        assert got[j].tobytes() == want.tobytes(), f"crop {j} (file {f} = rung {f // N}, row {f % N}, from sample {s}): differs from the oracle's decode of that file"
    assert (got[0] != got[1]).any() and (got[5] == 0).all()


def test_from_clips_ladder(codec):
    import torch
    import corpus
    bs, ch, enc, dec = codec
    T = ct.n_samples(bs)
    wave = torch.from_numpy(ct.wave(bs, ch)).to(_dev())
    rungs = (lt.VBR50, lt.AUTO96, lt.TABLE)
    refs = lt.refs(bs, ch, rungs)
    for layout in ("strided", "ragged"):
        cor = corpus.CropCorpus.from_clips_ladder(enc, dec, wave, ct.lengths(bs), rates=[(0, 50.0), ("auto", 96.0), np.array(ct.TABLE, np.float32)], layout=layout)
        assert cor.frozen and len(cor) == 3 * N and (cor.n_rungs, cor.n_clips) == (3, N) and cor.file_of(2, 5) == 2 * N + 5
        files = [cor.file_of(r, i) for r, i in ((0, 0), (0, 6), (1, 4), (1, 6), (2, 4), (2, 6))]
        pcm, _ = cor.sample_crops(dec, files, [bs] * len(files), T)
        torch.cuda.synchronize()
        pcm = pcm.cpu().numpy()
        for j, f in enumerate(files):
            want = _expected_crop(refs[f // N][f % N], bs, T)
            assert pcm[j].tobytes() == want.tobytes(), f"{layout}: file {f}: differs from the oracle's decode"
        assert cor.d_index_blocks.cpu().tolist() == [r.nb for g in refs for r in g]
        assert cor.avg.cpu().numpy().tobytes() == np.array([lt.avg(bs, ch, i) for i in range(N)], np.float32).tobytes()


def test_the_call_leaves_streaming_and_subset_state_alone(codec):
    """The call, with AUTO rungs, between the two halves of a streaming encode and of a subset encode on the same object: the
    streams' bytes stay the oracle's, and the call's files are what they are on a fresh object."""
    import torch
    bs, ch, enc, dec = codec
    enc.reset()
    pcm = np.stack([synth_pcm(40 + s, 4 * bs, ch, ct.RATE, transient=True, seed=3) for s in range(B)])
    slots = [5, 2, 7]

    def stream2(part):                                      # ulcx_encode_dev of two blocks of every stream
        d_pcm = torch.from_numpy(np.ascontiguousarray(part)).to(_dev())
        d_out = torch.zeros((B, 2, enc.slot), dtype=torch.uint8, device=_dev())
        d_bits = torch.zeros((B, 2), dtype=torch.int32, device=_dev())
        enc.encode_dev(d_pcm.data_ptr(), 2, d_out.data_ptr(), d_bits.data_ptr(), mode=0, p0=50.0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_bits.cpu().numpy()
    try:
        out1, bits1 = stream2(pcm[:, :2 * bs])
        a = LadderCall(enc, dec, bs, ch, lt.FIVE).run()
        out2, bits2 = stream2(pcm[:, 2 * bs:])
        out, bits = np.concatenate([out1, out2], 1), np.concatenate([bits1, bits2], 1)
        for s in range(B):
            ref = oracle_encode_debug(pcm[s], bs, ct.RATE, 0, 50.0, slot=enc.slot)
            assert np.array_equal(bits[s], ref["bits"]), (s, bits[s], ref["bits"])
            for k in range(4):
                assert np.array_equal(out[s, k, :bits[s, k] // 8], ref["out"][k, :bits[s, k] // 8]), f"stream {s} block {k}: the clips ladder call disturbed the stream"
        # a subset call's two halves (the shadow state is the subset calls' own) around the call: the slots go on with blocks 4 .. 7
        more = np.stack([synth_pcm(60 + s, 4 * bs, ch, ct.RATE, transient=True, seed=3) for s in slots])
        s1 = enc.encode_subset(slots, more[:, :2 * bs], mode=0, p0=50.0)
        b = LadderCall(enc, dec, bs, ch, lt.FIVE).run()
        s2 = enc.encode_subset(slots, more[:, 2 * bs:], mode=0, p0=50.0)
        for j, s in enumerate(slots):
            ref = oracle_encode_debug(np.concatenate([pcm[s], more[j]]), bs, ct.RATE, 0, 50.0, slot=enc.slot)
            so, sb = np.concatenate([s1[0][j], s2[0][j]]), np.concatenate([s1[1][j], s2[1][j]])
            assert np.array_equal(sb, ref["bits"][4:]), (s, sb, ref["bits"][4:])
            for k in range(4):
                assert np.array_equal(so[k, :sb[k] // 8], ref["out"][4 + k, :sb[k] // 8]), f"slot {s} block {4 + k}: the clips ladder call disturbed the subset call"
    finally:
        enc.reset()
    refs = lt.refs(bs, ch, lt.FIVE)
    check_files(a, refs, "between streaming calls")
    check_files(b, refs, "between subset calls")
    check_avg(a, bs, ch, "between streaming calls")
    check_avg(b, bs, ch, "between subset calls")


def test_host_form(codec):
    bs, ch, enc, dec = codec
    amd = _amd()
    table = np.array(ct.TABLE, np.float32)
    # The host form refuses AUTO on a table row that is VBR, and TABLE has three: its AUTO rung here is TABLE with those rows at
    # 96 kbps.  Their files are then AUTO 96's, the other rows' files AUTO on TABLE's: the same references.
    auto_table = table.copy()
    auto_table[table[:, 0] < 0] = (96.0, 7.0)               # (the table's own AvgComplexity is ignored)
    rungs = lt.lib_rungs(lt.FIVE[:4], table) + [("auto_table", auto_table)]
    payload, nbytes, maxb, index, count, avg = enc.encode_clips_ladder(dec, ct.wave(bs, ch), ct.lengths(bs), rungs=rungs)
    refs = lt.refs(bs, ch, lt.FIVE)
    refs[4] = [refs[3][i] if ct.TABLE[i][0] < 0 else refs[4][i] for i in range(N)]

    class Got:
        pass
    g = Got()
    g.n, g.R, g.pstride, g.istride = N, 5, payload.shape[2], index.shape[2]
    g.payload, g.nbytes, g.maxb, g.index, g.count = payload.reshape(5 * N, -1), nbytes.reshape(-1), maxb.reshape(-1), index.reshape(5 * N, -1), count.reshape(-1)
    g.poison = np.zeros_like(g.payload)                     # (the binding's own zeros: the host form writes the defined bytes only)
    check_files(g, refs, "host form")
    assert avg.tobytes() == np.array([lt.avg(bs, ch, i) for i in range(N)], np.float32).tobytes()
    assert table.tobytes() == np.array(ct.TABLE, np.float32).tobytes() and (auto_table[:, 1] == np.where(table[:, 0] < 0, 7.0, table[:, 1])).all()
    with pytest.raises(amd.UlcError, match="row 2 has -1 samples"):
        enc.encode_clips_ladder(dec, ct.wave(bs, ch), [1, 2, -1, 4, 5, 6, 7], rungs=[(0, 50.0)])
    bad = table.copy()
    bad[3, 0] = 0.0
    with pytest.raises(amd.UlcError, match="rung 1: invalid entry for row 3"):
        enc.encode_clips_ladder(dec, ct.wave(bs, ch), ct.lengths(bs), rungs=[(0, 50.0), bad])
    with pytest.raises(amd.UlcError, match="rung 0: ULCX_RUNG_AUTO on row 0, a VBR row"):
        enc.encode_clips_ladder(dec, ct.wave(bs, ch), ct.lengths(bs), rungs=[("auto_table", table)])
    with pytest.raises(amd.UlcError, match="rung 1: invalid setting, mode 1"):
        enc.encode_clips_ladder(dec, ct.wave(bs, ch), ct.lengths(bs), rungs=[(0, 50.0), (1, float("nan"))])
