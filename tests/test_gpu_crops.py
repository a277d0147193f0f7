"""Crops of a resident corpus on the GPU (include/ulc_amd.h section 3: ulcx_decode_crops_* / ulcx_index_packed_rows_*): every
row of a call names a file of the corpus and a block range of it.  Every comparison is bit for bit (int32 views) against the
oracle's sequential decode of the named file (tests/seek_testlib.py), never against this library's own decode; the indices
the calls are given come from the oracle too (its block sizes and generator states)."""
import ctypes as C
import functools
import numpy as np
import pytest

from ulc_testlib import same_bits, wc_of
from gpu_testlib import amd as _amd
from seek_testlib import ORACLE_BLOCKS, geometries, switched_starts, oracle_walk
from corpus_testlib import Corpus, geom_files, oracle_file, synth_file

pytestmark = pytest.mark.gpu
GEOMS = sorted(geometries().keys())
POISON_F, POISON_I = 7.0, 7


@functools.lru_cache(maxsize=None)
def _geom_corpus(geom):
    for (name, _, _, wc), f in zip(geometries()[geom], geom_files(geom)):
        if wc is not None:
            assert np.array_equal(f.wc, np.asarray(wc)), f"{name}: window codes read from the blocks differ from the oracle's"
    return Corpus(geom_files(geom))


FOUR = ((50.0, 3), (50.0, 4), (35.0, 5), (65.0, 6))         # (VBR quality, synth_pcm stream id) of four distinct 2048 x 2 streams


@functools.lru_cache(maxsize=None)
def _five_files():
    """Five distinct 2048 x 2 streams: oracle-encoded ids 3 .. 6 and the hand-assembled one."""
    return Corpus([oracle_file(2048, 2, q, sid) for q, sid in FOUR] + [synth_file(2048, 2)])


def _device_crops(dec, cor, files, first, N, count=None, pcm16=False, dev=None, keep=False):
    """ulcx_decode_crops_dev(_pcm16) on poisoned outputs -> (pcm [n][N][bs][ch], bits [n][N]) as numpy (keep: the device tensors)."""
    import torch
    d = dev or cor.to_device()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to("cuda:0")
    n = len(files)
    d_file, d_first = t(files), t(first)
    d_count = t(count) if count is not None else None
    pcm = torch.full((n, N, cor.bs, cor.ch), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full((n, N), POISON_I, dtype=torch.int32, device="cuda:0")
    dec.decode_crops_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                         n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr() if d_count is not None else 0, N,
                         pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return (pcm, bits) if keep else (pcm.cpu().numpy(), bits.cpu().numpy())


def _check_rows(cor, files, first, N, pcm, bits, what, count=None, rows=None):
    for i in (range(len(files)) if rows is None else rows):
        want, wb = cor.files[files[i]].expected_pcm(first[i], N, None if count is None else count[i])
        brow, prow = (bits[i].cpu().numpy(), pcm[i].cpu().numpy()) if hasattr(bits, "cpu") else (bits[i], pcm[i])
        assert np.array_equal(brow, wb), f"{what}: row {i} (file {files[i]} from block {first[i]}): bits {bits[i]} vs the oracle's {wb}"
        got = np.asarray(prow).reshape(N, cor.bs, cor.ch)
        for k in range(N):
            assert same_bits(got[k], want[k], shape=False), f"{what}: row {i}: block {first[i] + k} of file {files[i]} differs from the oracle's sequential decode"


# ---------------------------------------------------------------------------------------------------------------------
# 1. crops equal the oracle's slices
# ---------------------------------------------------------------------------------------------------------------------
def row_table(K, sw):
    """12 rows (file, first) over files of K[f] blocks, sw[f] = starts behind a window-switched block of file f: first 0, such
    starts, ranges running past the end, first == the block count, file 0 in six rows, one (file, first) pair twice."""
    a, z = 0, len(K) - 1
    pick = lambda f, i: sw[f][i % len(sw[f])]
    return [(a, 0), (a, pick(a, 0)), (a, pick(a, 1)), (a, K[a] - 3), (a, K[a]), (a, pick(a, 2)),
            (z, 0), (z, pick(z, 0)), (z, K[z] - 2), (a, pick(a, 0)), (z, K[z]), (z, 1)]


@pytest.mark.parametrize("geom", GEOMS)
def test_crops_equal_the_oracles_slices(geom):
    amd = _amd()
    bs, ch = geom
    cor = _geom_corpus(geom)
    st = geometries()[geom]
    sw = [switched_starts(wc_of(blocks)) for _, blocks, _, _ in st]
    for (name, _, _, wc), s in zip(st, sw):
        assert len(s) >= 3, f"{name}: {len(s)} starts behind a window-switched block"
    if geom == (2048, 2):
        assert cor.K == [40, 24]
    table = row_table(cor.K, sw)
    files, first = [f for f, _ in table], [k for _, k in table]
    assert len(table) == 12 and files.count(0) >= 4 and len(set(table)) < len(table)
    n, N = 12, 7
    dec = amd.BatchDecoder(16, ch, bs, N + 1)
    pcm, bits = dec.decode_crops(cor.host, cor.nbytes, cor.index, cor.count, files, first, N)          # the host form
    _check_rows(cor, files, first, N, pcm, bits, "host form")
    pcm, bits = _device_crops(dec, cor, files, first, N)
    _check_rows(cor, files, first, N, pcm, bits, "device form")
    dec.close()
    assert (bits > 0).sum() >= 6 * N


# ---------------------------------------------------------------------------------------------------------------------
# 2. more files than streams
# ---------------------------------------------------------------------------------------------------------------------
def test_a_corpus_of_more_files_than_the_decoder_has_streams():
    """A 2-stream decoder, a corpus of five distinct files.  A call has at most nStreams = 2 rows, so three calls (not two)
    name all five files; the sixth row takes file 0 again at another start."""
    amd = _amd()
    cor = _five_files()
    assert cor.F == 5
    N = 7
    dec = amd.BatchDecoder(2, cor.ch, cor.bs, N + 1)
    seen = set()
    for files, first in (([4, 1], [3, 30]), ([2, 3], [0, 11]), ([0, 0], [17, 36])):
        pcm, bits = _device_crops(dec, cor, files, first, N)
        _check_rows(cor, files, first, N, pcm, bits, f"files {files}")
        assert (bits[0] > 0).all()
        seen |= set(files)
    assert seen == set(range(5))
    with pytest.raises(amd.UlcError):                      # n is 1 .. nStreams
        _device_crops(dec, cor, [0, 1, 2], [0, 0, 0], N)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. d_count
# ---------------------------------------------------------------------------------------------------------------------
def test_counts_shorten_rows():
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    N = 7
    files, first = [0, 1, 0, 1, 0], [5, 9, 5, 20, 11]
    count = [0, 1, N, N + 3, 3]                            # (file 1 has 24 blocks: the row with N + 3 also runs past its end)
    dec = amd.BatchDecoder(8, cor.ch, cor.bs, N + 1)
    pcm, bits = _device_crops(dec, cor, files, first, N, count=count)
    _check_rows(cor, files, first, N, pcm, bits, "with counts", count=count)
    assert (bits[0] == 0).all() and (pcm[0] == 0).all() and bits[1, 0] > 0 and (bits[1, 1:] == 0).all() and (pcm[1, 1:] == 0).all()
    full, fbits = _device_crops(dec, cor, files, first, N)
    for i in (2, 3):                                       # a count of nBlocks or more: the row without one
        assert np.array_equal(bits[i], fbits[i]) and same_bits(pcm[i], full[i], shape=False), i
    hp, hb = dec.decode_crops(cor.host, cor.nbytes, cor.index, cor.count, files, first, N, count=count)
    assert np.array_equal(hb, bits) and same_bits(hp, pcm, shape=False), "host form with counts"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the object's state
# ---------------------------------------------------------------------------------------------------------------------
def test_crop_calls_leave_every_streams_state_untouched():
    """A decoder half-way through decode_packed of its own eight streams: crop calls under every launch plan reachable at that
    size (one workgroup per row; the even cut) change no byte of any slot's saved record, and the packed decode goes on as the
    oracle's.  The same around a range call and around subset calls (which share the compact state copy the crop call runs on)."""
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    bs, ch, B, NB = cor.bs, cor.ch, 8, 32
    pick = np.arange(B) % 2
    host, nbytes = np.ascontiguousarray(cor.host[pick]), cor.nbytes[pick]
    index, count = np.ascontiguousarray(cor.index[pick]), cor.count[pick]
    dec = amd.BatchDecoder(B, ch, bs, NB + 1)
    resident = dec.last_cut()[2]
    slots = list(range(B))
    cuts = set()

    def crops():
        for files, first, N in (([0, 1, 0], [3, 0, 20], 7), ([0, 1] * 4, [0, 1, 2, 3, 4, 5, 6, 7], NB)):
            pcm, bits = _device_crops(dec, cor, files, first, N)
            cuts.add(dec.last_cut()[0] > 0)
            _check_rows(cor, files, first, N, pcm, bits, f"crop call of {len(files)} x {N}", rows=(0, len(files) - 1))

    def packed(at, n, what):
        pcm, bits = dec.decode_packed(host, nbytes, n)
        for s in range(B):
            want, wb = cor.files[pick[s]].expected_pcm(at, n)
            assert np.array_equal(bits[s], wb) and same_bits(pcm[s], want, shape=False), f"{what}: stream {s}, blocks {at}.."

    packed(0, 6, "first half")
    before = dec.save_streams(slots)
    crops()
    after = dec.save_streams(slots)
    assert before.tobytes() == after.tobytes(), f"slots {sorted(set(np.argwhere(before != after)[:, 0].tolist()))} changed"
    assert cuts == ({False, True} if resident > 0 else {False}), (cuts, resident)
    packed(6, 6, "behind the crop calls")
    # around a range call: the state it leaves (a sequential decode up to its last block) survives crop calls
    first = np.array([15 if s % 2 == 0 else 9 for s in range(B)], np.int32)
    pcm, bits = dec.decode_range(host, nbytes, index, count, first, 4)
    before = dec.save_streams(slots)
    crops()
    assert before.tobytes() == dec.save_streams(slots).tobytes()
    pcm, bits = dec.decode_packed(host, nbytes, 3)
    for s in range(B):
        want, wb = cor.files[pick[s]].expected_pcm(first[s] + 4, 3)
        assert np.array_equal(bits[s], wb) and same_bits(pcm[s], want, shape=False), f"packed call behind range and crops: stream {s}"
    # around subset calls: slots 1, 4 and 6 decode slot-form blocks from the start, with crop calls between the two halves
    st = geometries()[(2048, 2)]
    sub = [1, 4, 6]
    dec.reset_streams(sub)
    blocks = np.stack([st[pick[s]][1][:8] for s in sub])
    pcm, bits = dec.decode_subset(sub, blocks[:, :4])
    before = dec.save_streams(slots)
    crops()
    assert before.tobytes() == dec.save_streams(slots).tobytes()
    pcm2, bits2 = dec.decode_subset(sub, blocks[:, 4:8])
    for i, s in enumerate(sub):
        want, wb = cor.files[pick[s]].expected_pcm(0, 8)
        got = np.concatenate([pcm[i].reshape(4, bs, ch), pcm2[i].reshape(4, bs, ch)])
        assert np.array_equal(np.concatenate([bits[i], bits2[i]]), wb) and same_bits(got, want, shape=False), f"subset calls around crops: slot {s}"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. agreement with the range call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_identity_crops_are_the_range_call(pcm16):
    import torch
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    B, N = cor.F, 7
    d = cor.to_device()
    dec, ref = amd.BatchDecoder(B, cor.ch, cor.bs, N + 1), amd.BatchDecoder(B, cor.ch, cor.bs, N + 1)
    sw = switched_starts(geometries()[(2048, 2)][0][3])
    for first in ([0, 0], [sw[0], 20], [37, 24], [41, 3]):
        d_first = torch.tensor(first, dtype=torch.int32, device="cuda:0")
        rp = torch.full((B, N, cor.bs, cor.ch), 7, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
        rb = torch.full((B, N), 7, dtype=torch.int32, device="cuda:0")
        ref.decode_range_dev(d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                             d_first.data_ptr(), N, rp.data_ptr(), rb.data_ptr(), pcm16=pcm16)
        torch.cuda.synchronize()
        pcm, bits = _device_crops(dec, cor, list(range(B)), first, N, pcm16=pcm16)
        assert np.array_equal(bits, rb.cpu().numpy()), first
        assert np.array_equal(pcm.view(np.int16 if pcm16 else np.int32), rp.cpu().numpy().view(np.int16 if pcm16 else np.int32)), first
        if first == [0, 0]:
            assert (bits > 0).all() and (pcm != 0).any()
    dec.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. bad rows
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_rows_are_silent_and_leave_their_neighbours_alone():
    import torch
    amd = _amd()
    cor = _geom_corpus((2048, 2))
    N, F = 7, cor.F
    # file 2: file 0 again, with the offset of its block 12 moved past its payload
    host = np.concatenate([cor.host, cor.host[:1]]); nbytes = np.concatenate([cor.nbytes, cor.nbytes[:1]])
    index = np.concatenate([cor.index, cor.index[:1]]); count = np.concatenate([cor.count, cor.count[:1]])
    index["ByteOffs"][2, 12] = int(nbytes[2]) + 1000
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    dev = dict(pay=t(host), nb=t(nbytes), idx=t(index.view(np.int32).reshape(3, -1)), cnt=t(count))
    files = [0, -1, 1, 3, 0, 1, 2, 2, 0, 1 << 30]
    first = [4, 4, 9, 0, -1, int(count[1]) + 1, 9, 20, 30, 0]
    bad = {1, 3, 4, 5, 6, 9}                                # (row 6 spans the moved entry; row 7, of the same file, does not)
    big = Corpus(cor.files + cor.files[:1])
    dec = amd.BatchDecoder(16, cor.ch, cor.bs, N + 1)
    pcm, bits = _device_crops(dec, big, files, first, N, dev=dev)
    for i in sorted(bad):
        assert (bits[i] == 0).all() and (pcm[i] == 0).all(), f"row {i} (file {files[i]}, first {first[i]}) is not silent"
    good = [i for i in range(len(files)) if i not in bad]
    _check_rows(big, files, first, N, pcm, bits, "beside bad rows", rows=good)
    assert all((bits[i] > 0).any() for i in good)
    # the host form refuses the first four (and a negative count) before any device work and leaves the outputs as they were
    L = amd.lib()
    i32 = lambda v: np.array(v, np.int32)
    for hf, h1, hc in (([0, -1], [0, 0], None), ([0, 3], [0, 0], None), ([0, 1], [0, -1], None), ([0, 1], [0, int(count[1]) + 1], None),
                       ([0, 1], [0, 0], [1, -1])):
        hp, hb = np.full((2, N * cor.bs, cor.ch), POISON_F, np.float32), np.full((2, N), POISON_I, np.int32)
        a = [i32(hf), i32(h1)] + ([i32(hc)] if hc else [])
        rc = L.ulcx_decode_crops_host(dec.h, 3, host.ctypes.data_as(C.POINTER(C.c_uint8)), host.shape[1], nbytes.ctypes.data_as(C.POINTER(C.c_int32)),
                                      index.ctypes.data, index.shape[1], count.ctypes.data_as(C.POINTER(C.c_int32)), 2,
                                      a[0].ctypes.data_as(C.POINTER(C.c_int32)), a[1].ctypes.data_as(C.POINTER(C.c_int32)),
                                      a[2].ctypes.data_as(C.POINTER(C.c_int32)) if hc else None, N,
                                      hp.ctypes.data_as(C.POINTER(C.c_float)), hb.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == -1, (hf, h1, hc)
        assert (hp == POISON_F).all() and (hb == POISON_I).all(), (hf, h1, hc)
    # the moved index entry is data, not an argument: the host form gives a silent row too
    hp, hb = dec.decode_crops(host, nbytes, index, count, [0, 2], [4, 9], N)
    assert (hb[1] == 0).all() and (hp[1] == 0).all() and (hb[0] > 0).all()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the cuts
# ---------------------------------------------------------------------------------------------------------------------
def test_few_long_crops_take_the_even_cut():
    amd = _amd()
    two = Corpus([oracle_file(2048, 2, 50.0, sid) for sid in (3, 4)])
    assert two.K == [40, 40]
    n, N = 8, 32
    dec = amd.BatchDecoder(n, two.ch, two.bs, N + 1)
    resident = dec.last_cut()[2]
    plan = amd.lib().ulcx_dec_split_plan(n, N, resident)
    assert resident > 0 and plan > 0, (resident, plan)
    files, first = [0, 1, 1, 0, 0, 1, 0, 1], [0, 8, 1, 5, 3, 0, 8, 12]
    pcm, bits = _device_crops(dec, two, files, first, N)
    assert dec.last_cut()[:2] == (plan, 0), dec.last_cut()
    _check_rows(two, files, first, N, pcm, bits, "even cut")
    dec.close()


def test_many_crops_take_the_cut_of_the_last_round():
    """resident + 2 resident / 3 rows of 24 blocks drawn from a corpus of FOUR files (nothing is replicated): whole rounds and a
    last round that is cut (ulcx_dec_range_tail_plan); rows of the whole rounds, of the cut round and at its edges."""
    amd = _amd()
    bs, ch, N = 2048, 2, 24
    probe = amd.BatchDecoder(8, ch, bs, N + 1)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0
    n = resident + resident * 2 // 3
    full = C.c_int32(0)
    tail = amd.lib().ulcx_dec_range_tail_plan(n, N, resident, C.byref(full))
    assert tail > 0 and full.value == resident, (n, resident, tail)
    cor = Corpus([oracle_file(bs, ch, q, sid) for q, sid in FOUR])
    rng = np.random.default_rng(21)
    files = rng.integers(0, 4, n).astype(np.int32)
    first = rng.integers(0, ORACLE_BLOCKS - N + 1, n).astype(np.int32)
    first[0], first[resident] = 0, 0
    first[n - 1] = ORACLE_BLOCKS - N + 5                    # the last row runs past its file's end
    dec = amd.BatchDecoder(n, ch, bs, N + 1)
    pcm, bits = _device_crops(dec, cor, files, first, N, keep=True)
    grid, whole, _ = dec.last_cut()
    assert (grid, whole) == (full.value + tail, full.value), (grid, whole, tail, full.value)
    _check_rows(cor, files, first, N, pcm, bits, "cut of the last round",
                rows=(0, 1, resident - 1, resident, resident + 1, resident + (n - resident) // 2, n - 2, n - 1))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the index with a row count of its own
# ---------------------------------------------------------------------------------------------------------------------
def test_index_packed_rows_of_a_one_stream_decoder():
    amd = _amd()
    cor = _five_files()
    one = amd.BatchDecoder(1, cor.ch, cor.bs, 2)
    index, count = one.index_packed_rows(cor.host, cor.nbytes, ORACLE_BLOCKS + 2)
    one.close()
    five = amd.BatchDecoder(5, cor.ch, cor.bs, 2)
    index5, count5 = five.index_packed(cor.host, cor.nbytes, ORACLE_BLOCKS + 2)
    five.close()
    assert np.array_equal(count, count5) and np.array_equal(index, index5)
    for f in range(cor.F):
        wbits, woffs, wseeds, inside = oracle_walk(cor.host[f], int(cor.nbytes[f]), cor.ch, cor.bs, ORACLE_BLOCKS + 2)
        n = len(wbits)
        assert inside and n == cor.K[f] == count[f], (f, n, count[f])
        assert np.array_equal(index["ByteOffs"][f, :n + 1], woffs) and np.array_equal(index["RngState"][f, :n + 1], wseeds), f
        assert (index["ByteOffs"][f, n + 1:] == -1).all() and (index["RngState"][f, n + 1:] == 0).all(), f
        assert np.array_equal(index[f, :n + 1], cor.index[f, :n + 1]), f


def test_crop_corpus_freezes_and_crops():
    """ulc-codec_amd/corpus.py end to end: two files with a stored `.ulx`, three indexed in freeze(); crops of float and PCM16."""
    import struct
    import torch
    import corpus
    amd = _amd()
    cor = _five_files()
    cc = corpus.CropCorpus(cor.ch, cor.bs)
    for f in range(cor.F):
        pay = cor.host[f, :cor.nbytes[f]].tobytes()
        ulc = struct.pack("<IHHIIHHI", 0x32434C55, cor.bs, 0, cor.K[f], 44100, cor.ch, 0, 24) + pay
        ulx = amd.ulx_pack(cor.index[f], cor.K[f], cor.bs, cor.ch, len(pay)) if f in (1, 3) else None
        assert cc.add_file(ulc, ulx) == f
    cc.freeze("cuda:0")
    assert np.array_equal(cc.d_index_blocks.cpu().numpy(), cor.count)
    got = cc.d_index.cpu().numpy().view(amd.INDEX_DTYPE).reshape(cor.F, -1)
    for f in range(cor.F):
        assert np.array_equal(got[f, :cor.K[f] + 1], cor.index[f, :cor.K[f] + 1]), f
    N = 7
    dec = amd.BatchDecoder(8, cor.ch, cor.bs, N + 1)
    files, first, count = [4, 0, 3, 3, 2, 1], [2, 33, 0, 0, 36, 12], [N, N, 4, N, N, 0]
    pcm, bits = cc.crops(dec, files, first, N, count=count)
    assert tuple(pcm.shape) == (6, N * cor.bs, cor.ch) and pcm.is_cuda
    torch.cuda.synchronize()
    _check_rows(cor, files, first, N, pcm.cpu().numpy(), bits.cpu().numpy(), "CropCorpus.crops", count=count)
    p16, b16 = cc.crops(dec, torch.tensor(files, dtype=torch.int32, device="cuda:0"), first, N, count=count, pcm16=True)
    want = torch.clamp(torch.round(pcm * 32768.0), -32768, 32767).to(torch.int16)
    assert torch.equal(b16, bits) and torch.equal(p16, want)
    dec.close()
