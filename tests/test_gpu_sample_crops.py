"""Sample crops on the GPU (include/ulc_amd.h section 3: ulcx_decode_crops_samples_*): row i of a call is nSamples samples from
sample d_start[i] of the decoded stream of file d_file[i], written channels-first, [n][nChan][nSamples].  Every comparison is
bit for bit (uint32 / int16 views) against the oracle's sequential decode of the named file (seek_testlib.oracle_pcm),
transposed and sliced in numpy - never against this library's own block-aligned crop call.  Streams and indices are the
oracle's (seek_testlib.geometries, oracle_stream, synth_stream; the corpora are test_gpu_crops.py's, built once per session)."""
import ctypes as C
import struct
import numpy as np
import pytest

from ulc_testlib import to_pcm16, same_bytes
from gpu_testlib import amd as _amd, word
import guarded_buffers as gb
from seek_testlib import geometries, switched_starts
from ulc_testlib import wc_of
from corpus_testlib import Corpus
from test_gpu_crops import _geom_corpus, _five_files

pytestmark = pytest.mark.gpu
GEOMS = sorted(geometries().keys())
POISON_F, POISON_I = 7.0, 7


def _blocks_of(bs, n_samples):
    return 1 + (n_samples + bs - 2) // bs


def expected_row(cor, f, start, n_samples, length=None, pcm16=False):
    """What row (f, start[, length]) must hold: the file's decoded stream [ch][K * bs] sliced at the sample, zeros behind the
    length and behind the file's end; the sizes of the blocks the row touches, 0 behind them and behind the file's end.  A file
    number out of range, a negative start and a start more than a block past the indexed blocks give zeros."""
    bs, ch = cor.bs, cor.ch
    nB = _blocks_of(bs, n_samples)
    out, bits = np.zeros((ch, n_samples), np.float32), np.zeros(nB, np.int32)
    ln = n_samples if length is None else max(0, min(n_samples, int(length)))
    if 0 <= f < cor.F and start >= 0 and start // bs <= cor.K[f] and ln > 0:
        pcm, rb = cor.files[f].pcm, cor.files[f].obits
        stream = pcm.reshape(cor.K[f] * bs, ch).T
        end = min(start + ln, cor.K[f] * bs)
        if end > start:
            out[:, :end - start] = stream[:, start:end]
        for b in range(start // bs, (start + ln - 1) // bs + 1):
            if b < cor.K[f]:
                bits[b - start // bs] = rb[b]
    return (to_pcm16(out) if pcm16 else out), bits


def _device_samples(dec, cor, files, start, n_samples, length=None, pcm16=False, dev=None):
    """ulcx_decode_crops_samples_dev(_pcm16) on poisoned outputs -> (pcm [n][ch][n_samples], bits [n][nB]) as numpy."""
    import torch
    d = dev or cor.to_device()
    n = len(files)
    d_file = torch.from_numpy(np.ascontiguousarray(files, np.int32)).to("cuda:0")
    d_start = torch.from_numpy(np.ascontiguousarray(start, np.int64)).to("cuda:0")
    d_len = torch.from_numpy(np.ascontiguousarray(length, np.int32)).to("cuda:0") if length is not None else None
    pcm = torch.full((n, cor.ch, n_samples), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full((n, _blocks_of(cor.bs, n_samples)), POISON_I, dtype=torch.int32, device="cuda:0")
    dec.decode_crops_samples_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                 n, d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr() if d_len is not None else 0, n_samples,
                                 pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), bits.cpu().numpy()


def _check_rows(cor, files, start, n_samples, pcm, bits, what, length=None, pcm16=False, rows=None):
    for i in (range(len(files)) if rows is None else rows):
        want, wb = expected_row(cor, int(files[i]), int(start[i]), n_samples, None if length is None else length[i], pcm16)
        where = f"{what}: row {i} (file {files[i]} from sample {start[i]}" + (f", length {length[i]})" if length is not None else ")")
        assert np.array_equal(bits[i], wb), f"{where}: bits {bits[i]} vs the oracle's {wb}"
        if not same_bytes(pcm[i], want):
            bad = np.argwhere(pcm[i].view(np.uint16 if pcm16 else np.uint32) != want.view(np.uint16 if pcm16 else np.uint32))
            raise AssertionError(f"{where}: {len(bad)} of {want.size} samples differ from the oracle's sequential decode, first at (channel, t) = "
                                 f"{bad[0].tolist()}, last at {bad[-1].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. every geometry, every store site's clip
# ---------------------------------------------------------------------------------------------------------------------
def row_table(bs, K, sw, n_samples):
    """Rows (file, start) over files of K[f] blocks; sw[f]: blocks directly behind a window-switched block of file f.  Starts 0, 1
    and bs - 1 (the crop straddles a boundary); an odd number of samples into a block behind a switched one and into the
    switched block itself (the decimated store sites clip at both ends of a crop); a crop that ends with the file's last
    sample, one that runs past it, one that starts at the file's end; one (file, start) twice; file 0 in more than six rows."""
    a, z = 0, len(K) - 1
    odd = (1, bs // 2 + 1, bs - 1, bs // 4 - 1)
    t = [(a, 0), (a, 1), (a, bs - 1)]
    for i, b in enumerate(sw[a][:4]):
        t += [(a, b * bs + odd[i % 4]), (a, (b - 1) * bs + odd[(i + 1) % 4])]
    t += [(z, sw[z][0] * bs + 3), (z, (sw[z][0] - 1) * bs + bs // 2 - 1)]
    t += [(a, max(0, K[a] * bs - n_samples)), (z, max(0, K[z] * bs - n_samples)),       # ends with the file's last sample
          (a, max(0, K[a] * bs - n_samples + (n_samples + 1) // 2)),                    # runs past the end: a zero tail
          (a, K[a] * bs), (z, K[z] * bs),                                               # starts at the end: all zero
          (a, 1), (z, 0)]
    return t


@pytest.mark.parametrize("geom", GEOMS)
def test_sample_crops_equal_the_oracles_slices(geom):
    amd = _amd()
    bs, ch = geom
    cor = _geom_corpus(geom)
    st = geometries()[geom]
    sw = [switched_starts(wc_of(blocks)) for _, blocks, _, _ in st]
    assert all(len(s) >= 3 for s in sw)
    sizes = (1, bs - 1, bs, bs + 1, 3 * bs + 5)
    dec = amd.BatchDecoder(32, ch, bs, _blocks_of(bs, max(sizes)) + 1)
    for n_samples in sizes:
        table = row_table(bs, cor.K, sw, n_samples)
        files, start = [f for f, _ in table], [s for _, s in table]
        assert files.count(0) >= 6 and len(set(table)) < len(table) and len(table) <= 32
        for pcm16 in (False, True):
            pcm, bits = _device_samples(dec, cor, files, start, n_samples, pcm16=pcm16)
            assert pcm.shape == (len(table), ch, n_samples)
            _check_rows(cor, files, start, n_samples, pcm, bits, f"{n_samples} samples, {'pcm16' if pcm16 else 'float'}", pcm16=pcm16)
            assert (bits[:3, 0] > 0).all() and (bits[-4] == 0).all() and (pcm[-4] == 0).all()
            assert n_samples < bs or (pcm[3:11] != 0).any(axis=(1, 2)).sum() >= 4      # (a stream may open with silence: the rows at the switched blocks)
        if n_samples == bs + 1:                             # the host form, once per geometry
            hp, hb = dec.decode_crops_samples(cor.host, cor.nbytes, cor.index, cor.count, files, start, n_samples)
            _check_rows(cor, files, start, n_samples, hp, hb, "host form")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. d_len
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (1024, 6)])
def test_lengths_shorten_rows(geom):
    amd = _amd()
    bs, ch = geom
    cor = _geom_corpus(geom)
    n_samples = 2 * bs + 3
    length = [0, 1, bs, n_samples, n_samples + 9, bs, 2]
    files = [0] * len(length)
    start = [5 * bs + 7, 5 * bs + 7, 3 * bs - 1, bs + 1, 2 * bs + 5, cor.K[0] * bs - 11, 4 * bs - 1]      # (row 5 also runs past the file's end)
    dec = amd.BatchDecoder(8, ch, bs, _blocks_of(bs, n_samples) + 1)
    for pcm16 in (False, True):
        pcm, bits = _device_samples(dec, cor, files, start, n_samples, length=length, pcm16=pcm16)
        _check_rows(cor, files, start, n_samples, pcm, bits, "with lengths", length=length, pcm16=pcm16)
        assert (bits[0] == 0).all() and (pcm[0] == 0).all()
        assert bits[1, 0] > 0 and (bits[1, 1:] == 0).all() and (pcm[1, :, 1:] == 0).all() and (pcm[1, :, 0] != 0).any()
        assert (bits[2, :2] > 0).all() and bits[2, 2] == 0 and (pcm[2, :, bs:] == 0).all()      # bs samples from bs - 1 into a block: two blocks
        assert (bits[6, :2] > 0).all() and bits[6, 2] == 0                                       # two samples across a boundary: two blocks
        full, fbits = _device_samples(dec, cor, files, start, n_samples, pcm16=pcm16)            # NULL d_len: every row takes nSamples
        _check_rows(cor, files, start, n_samples, full, fbits, "without lengths", pcm16=pcm16)
        for i in (3, 4):                                    # a length of nSamples or more: the row without one
            assert np.array_equal(bits[i], fbits[i]) and same_bytes(pcm[i], full[i]), i
    hp, hb = dec.decode_crops_samples(cor.host, cor.nbytes, cor.index, cor.count, files, start, n_samples, length=length)
    _check_rows(cor, files, start, n_samples, hp, hb, "host form with lengths", length=length)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the caller's buffers
# ---------------------------------------------------------------------------------------------------------------------
A_START, A_WORD = 8, 4
G_BS, G_CH, G_B, G_NS = 2048, 2, 8, 2 * 2048 + 1            # nSamples odd: every second plane starts off an 8-byte (float) / 4-byte (int16) boundary
G_ROWS = ([1, 0, 1, 0, 0, 2], [0, 3 * 2048 + 1, 24 * 2048 - 100, 7 * 2048 - 1, 40 * 2048, 5], [G_NS, 2048, G_NS, 1, G_NS, G_NS])   # row 2 past the end; row 5 a bad file


def _arena(cor, n, pcm16, with_len=True):
    F, stride = cor.host.shape
    esz = 2 if pcm16 else 4
    nB = _blocks_of(G_BS, G_NS)
    specs = [dict(name="d_payload", nbytes=F * stride, align=1, role="in", guard=F * stride, row=stride),
             word("d_payloadBytes", F, "in"),
             dict(name="d_index", nbytes=8 * F * cor.istride, align=A_WORD, role="in", guard=8 * F * cor.istride, row=8, rows_per_stream=cor.istride),
             word("d_indexBlocks", F, "in"), word("d_file", n, "in", G_B),
             dict(name="d_start", nbytes=8 * n, align=A_START, role="in", guard=8 * G_B, row=8)]
    if with_len:
        specs.append(word("d_len", n, "in", G_B))
    specs += [dict(name="d_pcm", nbytes=n * G_CH * G_NS * esz, align=esz, role="out", guard=G_B * G_CH * G_NS * esz, row=G_NS * esz, rows_per_stream=G_CH),
              word("d_bits", n * nB, "out", G_B * (nB + 1), nB)]
    a = gb.build(__import__("torch").device("cuda", 0), specs)
    a.load("d_payload", cor.host); a.load("d_payloadBytes", cor.nbytes); a.load("d_index", cor.index); a.load("d_indexBlocks", cor.count)
    return a


def _guarded_call(dec, cor, a, n, pcm16, off=None):
    p = lambda name: (a.ptr(name) + (off or {}).get(name, 0)) if name in a.regions else 0
    dec.decode_crops_samples_dev(cor.F, p("d_payload"), cor.host.shape[1], p("d_payloadBytes"), p("d_index"), cor.istride, p("d_indexBlocks"),
                                 n, p("d_file"), p("d_start"), p("d_len"), G_NS, p("d_pcm"), p("d_bits"), pcm16=pcm16)


def _guarded_check(cor, a, n, files, start, length, pcm16, what):
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, G_CH, G_NS)
    gbits = a.fetch("d_bits", np.int32).reshape(n, -1)
    _check_rows(cor, files, start, G_NS, got, gbits, what, length=length, pcm16=pcm16)


@pytest.mark.parametrize("with_len", [True, False], ids=["len", "no-len"])
@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_sample_crop_entries_on_poisoned_guarded_buffers(pcm16, with_len):
    """Every element of both outputs is written over the poison (the comparison is of whole rows, zeros included), nothing lands
    in a guard, no input changes.  d_pcm sits at an odd multiple of its element's size and a plane has an odd number of samples:
    no plane is aligned for a two-sample store by the carve's grace."""
    import torch
    amd = _amd()
    cor = _geom_corpus((G_BS, G_CH))
    files, start, length = G_ROWS
    n = len(files)
    a = _arena(cor, n, pcm16, with_len)
    assert a.ptr("d_pcm") % (4 if pcm16 else 8) != 0
    a.load("d_file", np.array(files, np.int32)); a.load("d_start", np.array(start, np.int64))
    if with_len:
        a.load("d_len", np.array(length, np.int32))
    dec = amd.BatchDecoder(G_B, G_CH, G_BS, _blocks_of(G_BS, G_NS) + 1)
    _guarded_call(dec, cor, a, n, pcm16)
    torch.cuda.synchronize()
    dec.close()
    a.check()
    _guarded_check(cor, a, n, files, start, length if with_len else None, pcm16, "guarded call")


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_misaligned_sample_crop_pointers_are_refused_and_nothing_is_touched(pcm16):
    """d_start off its 8 bytes, and each other pointer off its own alignment: ULCX_ERR_ARG before any device work - outputs keep
    their poison, every slot's saved record (a decoder in the middle of a packed decode) is byte-equal, and the next valid call
    is correct."""
    import torch
    amd = _amd()
    cor = _geom_corpus((G_BS, G_CH))
    files, start, length = G_ROWS
    n = len(files)
    a = _arena(cor, n, pcm16)
    a.load("d_file", np.array(files, np.int32)); a.load("d_start", np.array(start, np.int64)); a.load("d_len", np.array(length, np.int32))
    dec = amd.BatchDecoder(G_B, G_CH, G_BS, _blocks_of(G_BS, G_NS) + 1)
    pick = np.arange(G_B) % cor.F
    dec.decode_packed(cor.host[pick], cor.nbytes[pick], 2)
    before = dec.save_streams(list(range(G_B)))
    for name, by in (("d_start", 4), ("d_start", 2), ("d_len", 2), ("d_file", 1), ("d_pcm", 1 if pcm16 else 2), ("d_bits", 2), ("d_indexBlocks", 2)):
        with pytest.raises(amd.UlcError, match=r"\(-1\).*" + name + r".*not aligned"):
            _guarded_call(dec, cor, a, n, pcm16, off={name: by})
        assert amd.lib().ulcx_last_error().decode().startswith("ulcx_decode_crops_samples_dev" + ("_pcm16:" if pcm16 else ":"))
    torch.cuda.synchronize()
    a.check()
    assert a.fetch("d_pcm").tobytes() == gb.pattern(a.regions["d_pcm"].off, a.regions["d_pcm"].nbytes).tobytes(), "a refused call wrote samples"
    assert a.fetch("d_bits").tobytes() == gb.pattern(a.regions["d_bits"].off, a.regions["d_bits"].nbytes).tobytes(), "a refused call wrote sizes"
    assert before.tobytes() == dec.save_streams(list(range(G_B))).tobytes(), "a refused call changed a stream's state"
    _guarded_call(dec, cor, a, n, pcm16)
    torch.cuda.synchronize()
    a.check()
    _guarded_check(cor, a, n, files, start, length, pcm16, "valid call behind the refused ones")
    assert before.tobytes() == dec.save_streams(list(range(G_B))).tobytes(), "the sample-crop call changed a stream's state"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. cut launches: pieces of one row written by different workgroups
# ---------------------------------------------------------------------------------------------------------------------
def test_two_long_rows_take_the_even_cut():
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    bs, n = cor.bs, 2
    n_samples = 29 * bs + 1                                 # 30 blocks per row
    nB = _blocks_of(bs, n_samples)
    assert nB == 30 and amd.crop_blocks(bs, n_samples) == 30
    dec = amd.BatchDecoder(n, cor.ch, bs, nB + 1)
    resident = dec.last_cut()[2]
    plan = amd.lib().ulcx_dec_split_plan(n, nB, resident)
    assert resident > 0 and plan > n, (resident, plan)
    files, start = [0, 0], [9 * bs + 1001, 3 * bs]          # (the second row is block-aligned: its last block holds one sample of it)
    for pcm16 in (False, True):
        pcm, bits = _device_samples(dec, cor, files, start, n_samples, pcm16=pcm16)
        assert dec.last_cut()[:2] == (plan, 0), dec.last_cut()     # more workgroups than rows: every row is in pieces
        _check_rows(cor, files, start, n_samples, pcm, bits, "even cut", pcm16=pcm16)
        assert (bits[0] > 0).all() and (bits[1] > 0).all()
    dec.close()


def test_many_rows_take_the_cut_of_the_last_round():
    """resident + 2 resident / 3 rows of 6 blocks: whole rounds of one workgroup per row, and a last round whose rows are cut
    into pieces (ulcx_dec_range_tail_plan).  Rows of the whole rounds, of the cut round and at its edges."""
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    bs, ch = cor.bs, cor.ch
    n_samples = 4 * bs + 2
    nB = _blocks_of(bs, n_samples)
    assert nB == 6
    probe = amd.BatchDecoder(8, ch, bs, nB + 1)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0
    n = resident + resident * 2 // 3
    full = C.c_int32(0)
    tail = amd.lib().ulcx_dec_range_tail_plan(n, nB, resident, C.byref(full))
    assert tail > n - resident and full.value == resident, (n, resident, tail)
    rng = np.random.default_rng(33)
    files = rng.integers(0, cor.F, n).astype(np.int32)
    start = np.array([rng.integers(0, cor.K[f] * bs - n_samples) for f in files], np.int64)
    start[0], start[resident], start[n - 1] = 0, bs - 1, cor.K[files[n - 1]] * bs - n_samples // 2       # the last row runs past its file's end
    dec = amd.BatchDecoder(n, ch, bs, nB + 1)
    pcm, bits = _device_samples(dec, cor, files, start, n_samples)
    grid, whole, _ = dec.last_cut()
    assert (grid, whole) == (full.value + tail, full.value), (grid, whole, tail, full.value)
    _check_rows(cor, files, start, n_samples, pcm, bits, "cut of the last round",
                rows=(0, 1, resident - 1, resident, resident + 1, resident + (n - resident) // 2, n - 2, n - 1))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. ragged == strided, through corpus.py
# ---------------------------------------------------------------------------------------------------------------------
def test_ragged_and_strided_corpora_give_the_same_sample_crops():
    import torch
    import corpus
    amd = _amd()
    cor = _five_files()
    ccs = {}
    for layout in ("strided", "ragged"):
        cc = corpus.CropCorpus(cor.ch, cor.bs, layout=layout)
        for f in range(cor.F):
            pay = cor.host[f, :cor.nbytes[f]].tobytes()
            ulc = struct.pack("<IHHIIHHI", 0x32434C55, cor.bs, 0, cor.K[f], 44100, cor.ch, 0, 24) + pay
            ulx = amd.ulx_pack(cor.index[f], cor.K[f], cor.bs, cor.ch, len(pay)) if f in (1, 3) else None
            assert cc.add_file(ulc, ulx) == f
        ccs[layout] = cc.freeze("cuda:0")
    bs = cor.bs
    n_samples = 3 * bs + 5
    files = [4, 0, 3, 3, 2, 1, 4]
    start = [2 * bs + 1, 33 * bs + 77, 0, bs - 1, 36 * bs + 5, 12 * bs + 1023, 24 * bs]        # (file 4 has 24 blocks: the last row is all zero)
    length = [n_samples, n_samples, 4, n_samples, n_samples, 0, n_samples]
    dec = amd.BatchDecoder(8, cor.ch, bs, amd.crop_blocks(bs, n_samples) + 1)
    for pcm16 in (False, True):
        got = {}
        for layout, cc in ccs.items():
            pcm, bits = cc.sample_crops(dec, files, torch.tensor(start, dtype=torch.int64, device="cuda:0"), n_samples, length=length, pcm16=pcm16)
            assert tuple(pcm.shape) == (len(files), cor.ch, n_samples) and pcm.is_cuda and pcm.is_contiguous()
            torch.cuda.synchronize()
            got[layout] = (pcm.cpu().numpy(), bits.cpu().numpy())
            _check_rows(cor, files, start, n_samples, *got[layout], f"CropCorpus({layout}).sample_crops", length=length, pcm16=pcm16)
        assert same_bytes(got["strided"][0], got["ragged"][0]) and np.array_equal(got["strided"][1], got["ragged"][1])
    hp, hb = dec.decode_crops_samples_ragged(ccs["ragged"].d_payload.cpu().numpy(), ccs["ragged"].d_payload_offs.cpu().numpy(),
                                             ccs["ragged"].d_index.cpu().numpy().view(amd.INDEX_DTYPE).reshape(-1), ccs["ragged"].d_index_offs.cpu().numpy(),
                                             cor.count, files, start, n_samples, length=length)
    _check_rows(cor, files, start, n_samples, hp, hb, "ragged host form", length=length)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the object's state
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_crops_between_two_halves_of_a_packed_decode():
    """A decoder half-way through decode_packed of its own eight streams: sample-crop calls under both launch plans reachable at
    that size change no byte of any slot's saved record, and the packed decode goes on as the oracle's uninterrupted one."""
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    bs, ch, B = cor.bs, cor.ch, 8
    long_ns = 23 * bs + 9
    pick = np.arange(B) % 2
    host, nbytes = np.ascontiguousarray(cor.host[pick]), cor.nbytes[pick]
    dec = amd.BatchDecoder(B, ch, bs, _blocks_of(bs, long_ns) + 1)
    resident = dec.last_cut()[2]
    slots = list(range(B))

    def packed(at, n, what):
        pcm, bits = dec.decode_packed(host, nbytes, n)
        for s in range(B):
            want, wb = cor.files[pick[s]].expected_pcm(at, n)
            assert np.array_equal(bits[s], wb) and same_bytes(np.asarray(pcm[s], np.float32).reshape(want.shape), want), f"{what}: stream {s}, blocks {at}.."

    packed(0, 6, "first half")
    before = dec.save_streams(slots)
    cuts = set()
    for files, start, n_samples in (([0, 1, 0], [3 * bs + 1, 0, 20 * bs + 999], 2 * bs + 1), ([0, 1] * 4, [k * bs + 17 * k for k in range(8)], long_ns)):
        pcm, bits = _device_samples(dec, cor, files, start, n_samples)
        cuts.add(dec.last_cut()[0] > 0)
        _check_rows(cor, files, start, n_samples, pcm, bits, f"sample crops of {len(files)} x {n_samples}")
    assert before.tobytes() == dec.save_streams(slots).tobytes(), "a sample-crop call changed a stream's state"
    assert cuts == ({False, True} if resident > 0 else {False}), (cuts, resident)
    packed(6, 6, "behind the sample-crop calls")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. untrusted rows
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_rows_are_silent_and_leave_their_neighbours_alone():
    import torch
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    bs, F = cor.bs, cor.F
    n_samples = 2 * bs + 3
    # file 2: file 0 again, with the offset of its block 12 moved past its payload
    host = np.concatenate([cor.host, cor.host[:1]]); nbytes = np.concatenate([cor.nbytes, cor.nbytes[:1]])
    index = np.concatenate([cor.index, cor.index[:1]]); count = np.concatenate([cor.count, cor.count[:1]])
    index["ByteOffs"][2, 12] = int(nbytes[2]) + 1000
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    dev = dict(pay=t(host), nb=t(nbytes), idx=t(index.view(np.int32).reshape(3, -1)), cnt=t(count))
    big = Corpus(cor.files + cor.files[:1])
    K1 = cor.K[1]
    files = [0, -1, 1, 3, 0, 1, 2, 2, 0, 1 << 30, 0, 1]
    start = [4 * bs + 5, 4 * bs, 9 * bs + 1, 0, -1, (K1 + 1) * bs, 10 * bs + 9, 20 * bs + 1, 30 * bs, 0, -(1 << 40), (1 << 45) + 7]
    bad = {1, 3, 4, 5, 6, 9, 10, 11}                        # (row 6 spans the moved entry; row 7, of the same file, does not)
    dec = amd.BatchDecoder(16, cor.ch, bs, _blocks_of(bs, n_samples) + 1)
    for pcm16 in (False, True):
        pcm, bits = _device_samples(dec, big, files, start, n_samples, dev=dev, pcm16=pcm16)
        for i in sorted(bad):
            assert (bits[i] == 0).all() and (pcm[i] == 0).all(), f"row {i} (file {files[i]}, start {start[i]}) is not silent"
        good = [i for i in range(len(files)) if i not in bad]
        _check_rows(big, files, start, n_samples, pcm, bits, "beside bad rows", rows=good, pcm16=pcm16)
        assert all((bits[i, :3] > 0).all() and bits[i, 3] == 0 and (pcm[i] != 0).any() for i in good)
    # the host forms refuse what the device forms cannot, before any device work, under their own name
    L = amd.lib()
    i32p, i64p, u8p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    poffs = np.arange(4, dtype=np.int64) * host.shape[1]
    ioffs = np.arange(4, dtype=np.int64) * index.shape[1]
    cases = (([0, -1], [0, 0], None), ([0, 3], [0, 0], None), ([0, 1], [0, -1], None), ([0, 1], [0, K1 * bs + 1], None), ([0, 1], [0, 0], [1, -1]))
    for hf, hs, hl in cases:
        for ragged in (False, True):
            name = "ulcx_decode_crops_samples_ragged_host" if ragged else "ulcx_decode_crops_samples_host"
            hp, hb = np.full((2, cor.ch, n_samples), POISON_F, np.float32), np.full((2, _blocks_of(bs, n_samples)), POISON_I, np.int32)
            a = [np.array(hf, np.int32), np.array(hs, np.int64)] + ([np.array(hl, np.int32)] if hl else [])
            rows = (2, a[0].ctypes.data_as(i32p), a[1].ctypes.data_as(i64p), a[2].ctypes.data_as(i32p) if hl else None, n_samples,
                    hp.ctypes.data_as(f32p), hb.ctypes.data_as(i32p))
            if ragged:
                rc = L.ulcx_decode_crops_samples_ragged_host(dec.h, 3, host.ctypes.data_as(u8p), host.size, poffs.ctypes.data_as(i64p), index.ctypes.data,
                                                             index.size, ioffs.ctypes.data_as(i64p), count.ctypes.data_as(i32p), *rows)
            else:
                rc = L.ulcx_decode_crops_samples_host(dec.h, 3, host.ctypes.data_as(u8p), host.shape[1], nbytes.ctypes.data_as(i32p), index.ctypes.data,
                                                      index.shape[1], count.ctypes.data_as(i32p), *rows)
            assert rc == -1, (name, hf, hs, hl)
            assert L.ulcx_last_error().decode().startswith(name + ": row 1 "), L.ulcx_last_error().decode()
            assert (hp == POISON_F).all() and (hb == POISON_I).all(), (name, hf, hs, hl)
    # a start of exactly indexBlocks * BlockSize is a row of zeros, not a refusal; the moved index entry is data, not an argument
    hp, hb = dec.decode_crops_samples(host, nbytes, index, count, [0, 2, 1], [4 * bs + 5, 10 * bs + 9, K1 * bs], n_samples)
    assert (hb[1] == 0).all() and (hp[1] == 0).all() and (hb[2] == 0).all() and (hp[2] == 0).all() and (hb[0, :3] > 0).all()
    _check_rows(big, [0], [4 * bs + 5], n_samples, hp, hb, "host form beside bad rows")
    dec.close()
