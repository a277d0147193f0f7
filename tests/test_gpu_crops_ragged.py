"""Crops of a ragged corpus on the GPU (include/ulc_amd.h section 3: ulcx_decode_crops_ragged_* / ulcx_index_packed_ragged_*): the
files lie back to back at their own length, found through two int64 offset tables.  Every expectation is the oracle's
sequential decode of the named file, or the oracle's walk of its payload (tests/seek_testlib.py, tests/ragged_testlib.py), bit
for bit; where the header promises equality with the strided calls, that is compared as well."""
import ctypes as C
import functools
import struct
import numpy as np
import pytest

from gpu_testlib import amd as _amd, to_dev as _t, word
import guarded_buffers as gb
from seek_testlib import damaged, oracle_walk
from ulc_testlib import to_pcm16, same_bytes
from corpus_testlib import INDEX_DTYPE, PAD, Corpus
from ragged_testlib import FILE_BLOCKS, GEOMS, file_refs

pytestmark = pytest.mark.gpu
STEREO = (2048, 2)
POISON_F, POISON_I = 7.0, 7
N = 5                                                      # blocks per row of the crop calls here


@functools.lru_cache(maxsize=None)
def _corpus(geom):
    return Corpus(file_refs(geom))


@functools.lru_cache(maxsize=None)
def _on_device(geom):
    cor = _corpus(geom)
    d = cor.to_device()
    return dict(pay=d["rpay"], poffs=d["poffs"], idx=d["ridx"], ioffs=d["ioffs"], cnt=d["cnt"],
                s_pay=d["pay"], s_nb=d["nb"], s_idx=d["idx"], s_stride=cor.stride, s_istride=cor.istride)


def _ragged_dev(dec, cor, d, files, first, n_blocks, count=None, pcm16=False):
    """ulcx_decode_crops_ragged_dev(_pcm16) on poisoned outputs -> (pcm [n][n_blocks][bs][ch], bits [n][n_blocks]) as numpy"""
    import torch
    ref = file_refs(STEREO)[0] if cor is None else next(f for f in cor.files if f is not None)
    n = len(files)
    d_file, d_first = _t(files, np.int32), _t(first, np.int32)
    d_count = _t(count, np.int32) if count is not None else None
    pcm = torch.full((n, n_blocks, ref.bs, ref.ch), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full((n, n_blocks), POISON_I, dtype=torch.int32, device="cuda:0")
    dec.decode_crops_ragged_dev(d["cnt"].numel(), d["pay"].data_ptr(), d["pay"].numel(), d["poffs"].data_ptr(), d["idx"].data_ptr(), d["idx"].numel() // 2,
                                d["ioffs"].data_ptr(), d["cnt"].data_ptr(), n, d_file.data_ptr(), d_first.data_ptr(),
                                d_count.data_ptr() if d_count is not None else 0, n_blocks, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), bits.cpu().numpy()


def _assert_rows(got, gbits, want, wbits, files, first, what, rows=None):
    for i in (range(len(files)) if rows is None else rows):
        assert np.array_equal(gbits[i], wbits[i]), f"{what}: row {i} (file {files[i]} from block {first[i]}): bits {gbits[i]} vs the oracle's {wbits[i]}"
        assert same_bytes(got[i], want[i], shape=False), f"{what}: row {i} (file {files[i]} from block {first[i]}): samples differ from the oracle's sequential decode"


# (file, first, count) over files of 1, 2, 7, 12 and 40 blocks: start 0; start at the last block; start equal to the block count
# (a zero row); ranges running past the end; file 4 in three rows (one start twice); counts of 0, 1 and N
ROWS = [(4, 0, N), (0, 0, N), (4, 39, N), (2, 6, N), (3, 12, N), (0, 1, N), (3, 9, N), (1, 1, N), (4, 10, N), (4, 10, N), (4, 33, N),
        (4, 5, 0), (2, 2, 1), (3, 3, N)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. ragged crops equal the oracle's slices, and the strided call on the strided copy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_ragged_crops_equal_the_oracles_slices_and_the_strided_call(geom, pcm16):
    import torch
    amd = _amd()
    bs, ch = geom
    cor, d = _corpus(geom), _on_device(geom)
    assert tuple(f.K for f in cor.files) == FILE_BLOCKS == (1, 2, 7, 12, 40)
    files, first, count = [r[0] for r in ROWS], [r[1] for r in ROWS], [r[2] for r in ROWS]
    n = len(ROWS)
    dec = amd.BatchDecoder(16, ch, bs, N + 1)
    for cnt in (count, None):
        want, wbits = cor.expected_pcm(files, first, N, cnt)
        assert (wbits[4] == 0).all() and (wbits[5] == 0).all() and (wbits[0] > 0).all() and wbits[2, 0] > 0 and (wbits[2, 1:] == 0).all()
        if pcm16:
            want = to_pcm16(want)
        got, gbits = _ragged_dev(dec, cor, d, files, first, N, cnt, pcm16)
        _assert_rows(got, gbits, want, wbits, files, first, f"ragged, {'counts' if cnt else 'no counts'}")
        # the strided call on the strided copy of the same corpus
        sp = torch.full((n, N, bs, ch), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
        sb = torch.full((n, N), POISON_I, dtype=torch.int32, device="cuda:0")
        d_count = _t(cnt, np.int32) if cnt is not None else None
        d_file, d_first = _t(files, np.int32), _t(first, np.int32)
        dec.decode_crops_dev(cor.F, d["s_pay"].data_ptr(), d["s_stride"], d["s_nb"].data_ptr(), d["s_idx"].data_ptr(), d["s_istride"], d["cnt"].data_ptr(),
                             n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr() if cnt is not None else 0, N,
                             sp.data_ptr(), sb.data_ptr(), pcm16=pcm16)
        torch.cuda.synchronize()
        assert np.array_equal(gbits, sb.cpu().numpy()) and same_bytes(got, sp.cpu().numpy(), shape=False), "ragged and strided calls differ"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the host form
# ---------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_the_device_form():
    amd = _amd()
    cor, d = _corpus(STEREO), _on_device(STEREO)
    rows = [r for r in ROWS if r[1] <= FILE_BLOCKS[r[0]]]
    files, first, count = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    dec = amd.BatchDecoder(16, 2, 2048, N + 1)
    for cnt in (count, None):
        got, gbits = _ragged_dev(dec, cor, d, files, first, N, cnt)
        hp, hb = dec.decode_crops_ragged(cor.rpay, cor.poffs, cor.ridx, cor.ioffs, cor.count, files, first, N, count=cnt)
        assert np.array_equal(hb, gbits) and same_bytes(hp.reshape(got.shape), got, shape=False)
        want, wbits = cor.expected_pcm(files, first, N, cnt)
        _assert_rows(hp.reshape(got.shape), hb, want, wbits, files, first, "host form")
    # what the strided host form refuses: a file number out of range, a start behind the file's blocks, a negative count
    for hf, h1, hc in (([0, 5], [0, 0], None), ([0, -1], [0, 0], None), ([0, 3], [0, 13], None), ([0, 3], [0, -1], None), ([0, 3], [0, 0], [1, -1])):
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            dec.decode_crops_ragged(cor.rpay, cor.poffs, cor.ridx, cor.ioffs, cor.count, hf, h1, N, count=hc)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the object's state
# ---------------------------------------------------------------------------------------------------------------------
def test_ragged_crop_calls_leave_every_streams_state_untouched():
    """A decoder in the middle of a ulcx_decode_packed_dev sequence over its own eight streams: ragged crop calls under both
    launch plans reachable at that size (one workgroup per row; the even cut) change no byte of any slot's saved record, and the
    packed decode goes on as the oracle's."""
    import torch
    amd = _amd()
    cor, d = _corpus(STEREO), _on_device(STEREO)
    bs, ch, B, NB = 2048, 2, 8, 32
    pick = [3, 4] * 4                                       # the files of 12 and 40 blocks, as streams of the object
    host, nbytes = cor.host, cor.nbytes
    d_pay, d_nb = _t(host[pick]), _t(nbytes[pick])
    dec = amd.BatchDecoder(B, ch, bs, NB + 1)
    resident = dec.last_cut()[2]
    slots = list(range(B))
    cuts = set()

    def packed(at, n, what):
        pcm = torch.full((B, n, bs, ch), POISON_F, dtype=torch.float32, device="cuda:0")
        bits = torch.full((B, n), POISON_I, dtype=torch.int32, device="cuda:0")
        dec.decode_packed_dev(d_pay.data_ptr(), host.shape[1], d_nb.data_ptr(), n, pcm.data_ptr(), bits.data_ptr())
        torch.cuda.synchronize()
        want, wbits = cor.expected_pcm(pick, [at] * B, n)
        _assert_rows(pcm.cpu().numpy(), bits.cpu().numpy(), want, wbits, pick, [at] * B, what)

    packed(0, 4, "first call of the sequence")
    before = dec.save_streams(slots)
    for files, first, nb in (([4, 3, 0], [3, 0, 0], 7), ([4, 3] * 4, [0, 1, 2, 3, 4, 5, 6, 7], NB)):
        got, gbits = _ragged_dev(dec, cor, d, files, first, nb)
        cuts.add(dec.last_cut()[0] > 0)
        want, wbits = cor.expected_pcm(files, first, nb)
        _assert_rows(got, gbits, want, wbits, files, first, f"crop call of {len(files)} x {nb}")
    after = dec.save_streams(slots)
    assert before.tobytes() == after.tobytes(), f"slots {sorted(set(np.argwhere(before != after)[:, 0].tolist()))} changed"
    assert cuts == ({False, True} if resident > 0 else {False}), (cuts, resident)
    packed(4, 4, "behind the crop calls")
    assert (dec.save_streams(slots) != before).any()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. untrusted tables, one bad file at a time
# ---------------------------------------------------------------------------------------------------------------------
BAD = 4                                                    # the file of 12 blocks, between two files nobody crops
CASES = ("end-before-start", "negative-start", "end-past-total", "2^31-bytes", "capacity-below-blocks+1", "index-offset-past-total",
         "closing-entry-past-size")
OFFSET_TABLE_CASES = CASES[:4] + CASES[5:6]


@functools.lru_cache(maxsize=None)
def _guarded_corpus():
    """Files of 1, 2 and 7 blocks, a file nobody crops, the file of 12 blocks, another such file, the file of 40: an offset of
    file 4 is an offset of a neighbour too (the end of one file is the start of the next), and the neighbours have no rows."""
    r = file_refs(STEREO)
    return Corpus([r[0], r[1], r[2], None, r[3], None, r[4]])


def _guards_2g(total, cor):
    """The 2^31-bytes case needs a payload buffer of more than 2^31 bytes: uninitialised device memory with the files' bytes at
    its start and a guard of the arena's pattern on either side.  -> (tensor, address of the buffer, check())"""
    import torch
    G = 1 << 16
    t = torch.empty(G + total + G, dtype=torch.uint8, device="cuda:0")
    t[:G] = _t(gb.pattern(0, G)); t[G + total:] = _t(gb.pattern(G + total, G))
    t[G:G + cor.rpay.size] = _t(cor.rpay)

    def check():
        assert t[:G].cpu().numpy().tobytes() == gb.pattern(0, G).tobytes(), "leading guard of d_payload written"
        assert t[G + total:].cpu().numpy().tobytes() == gb.pattern(G + total, G).tobytes(), "trailing guard of d_payload written"
        assert t[G:G + cor.rpay.size].cpu().numpy().tobytes() == cor.rpay.tobytes(), "d_payload modified"
    return t, t.data_ptr() + G, check


@pytest.mark.parametrize("case", CASES)
def test_untrusted_tables_silence_one_file_and_leave_the_others(case):
    import torch
    amd = _amd()
    cor = _guarded_corpus()
    bs, ch, F = 2048, 2, cor.F
    poffs, ioffs, index = cor.poffs.copy(), cor.ioffs.copy(), cor.ridx.copy()
    ptotal, itotal = cor.rpay.size, index.size
    size = int(poffs[BAD + 1] - poffs[BAD])
    if case == "end-before-start":
        poffs[BAD + 1] = poffs[BAD] - 1
    elif case == "negative-start":
        poffs[BAD] = -16
    elif case == "end-past-total":
        poffs[BAD + 1] = ptotal + 1
    elif case == "2^31-bytes":
        ptotal = int(poffs[BAD]) + (1 << 31) + 4096
        poffs[BAD + 1] = poffs[BAD] + (1 << 31)
    elif case == "capacity-below-blocks+1":
        ioffs[BAD + 1] = ioffs[BAD] + 12
    elif case == "index-offset-past-total":
        ioffs[BAD + 1] = itotal + 3
    else:
        index["ByteOffs"][ioffs[BAD] + 12] = size + 1
    # rows of the bad file (all of them reach its closing entry in the last case: an index entry is looked at by the rows whose
    # blocks it bounds, as in the strided call) between rows of every other file
    bad_rows = [(BAD, 8), (BAD, 10), (BAD, 12)] if case == "closing-entry-past-size" else [(BAD, 0), (BAD, 10), (BAD, 12)]
    table = [(6, 0), bad_rows[0], (2, 3), (6, 36), bad_rows[1], (1, 0), (0, 0), bad_rows[2], (6, 17)]
    files, first = [f for f, _ in table], [k for _, k in table]
    n, B, MAXK = len(table), 12, 8
    row = bs * ch * 4
    specs = [dict(name="d_payloadOffs", nbytes=8 * (F + 1), align=8, role="in", guard=8 * (F + 1), row=8),
             dict(name="d_index", nbytes=8 * index.size, align=4, role="in", guard=8 * index.size, row=8),
             dict(name="d_indexOffs", nbytes=8 * (F + 1), align=8, role="in", guard=8 * (F + 1), row=8),
             word("d_indexBlocks", F, "in"), word("d_file", n, "in", B), word("d_first", n, "in", B),
             dict(name="d_pcm", nbytes=n * N * row, align=16, role="out", guard=B * MAXK * row, row=row, rows_per_stream=N),
             word("d_bits", n * N, "out", B * MAXK, N)]
    big = case == "2^31-bytes"
    if not big:
        specs.insert(0, dict(name="d_payload", nbytes=ptotal, align=1, role="in", guard=ptotal, row=ptotal))
    a = gb.build(torch.device("cuda", 0), specs)
    if big:
        try:
            keep, pay_ptr, pay_check = _guards_2g(ptotal, cor)
        except (RuntimeError, MemoryError) as e:
            pytest.skip(f"no {ptotal} bytes of device memory for the payload buffer: {e}")
    else:
        a.load("d_payload", cor.rpay)
        pay_ptr, pay_check = a.ptr("d_payload"), lambda: None
    a.load("d_payloadOffs", poffs); a.load("d_index", index); a.load("d_indexOffs", ioffs); a.load("d_indexBlocks", cor.count)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32))
    dec = amd.BatchDecoder(B, ch, bs, MAXK)
    dec.decode_crops_ragged_dev(F, pay_ptr, ptotal, a.ptr("d_payloadOffs"), a.ptr("d_index"), itotal, a.ptr("d_indexOffs"), a.ptr("d_indexBlocks"),
                                n, a.ptr("d_file"), a.ptr("d_first"), 0, N, a.ptr("d_pcm"), a.ptr("d_bits"))
    torch.cuda.synchronize()
    a.check(); pay_check()
    got = a.fetch("d_pcm", np.float32).reshape(n, N, bs, ch)
    gbits = a.fetch("d_bits", np.int32).reshape(n, N)
    want, wbits = cor.expected_pcm(files, first, N)
    silent = [i for i, (f, _) in enumerate(table) if f == BAD]
    good = [i for i in range(n) if i not in silent]
    assert all((wbits[i] > 0).any() for i in good) and (wbits[silent[0]] > 0).any()
    for i in silent:
        assert (gbits[i] == 0).all() and not got[i].any(), f"{case}: row {i} (file {files[i]} from block {first[i]}) is not silent"
    _assert_rows(got, gbits, want, wbits, files, first, f"{case}: beside the bad file", rows=good)
    # the host form: an offset table it can see through is refused before any device work, nothing of the outputs or the
    # object touched; an index that does not fit its file is data, and gives the silent rows of the device form
    slots = list(range(B))
    before = dec.save_streams(slots)
    payload = np.empty(ptotal, np.uint8) if big else cor.rpay          # (refused before a byte of it is looked at)
    hf, h1 = [f for f, _ in table[:6]], [k for _, k in table[:6]]
    if case in OFFSET_TABLE_CASES:
        hp, hb = np.full((6, N * bs, ch), POISON_F, np.float32), np.full((6, N), POISON_I, np.int32)
        i32, i64 = lambda v: np.ascontiguousarray(v, np.int32), C.POINTER(C.c_int64)
        af, a1 = i32(hf), i32(h1)
        rc = amd.lib().ulcx_decode_crops_ragged_host(dec.h, F, payload.ctypes.data_as(C.POINTER(C.c_uint8)), ptotal, poffs.ctypes.data_as(i64),
                                                     index.ctypes.data, itotal, ioffs.ctypes.data_as(i64), cor.count.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     6, af.ctypes.data_as(C.POINTER(C.c_int32)), a1.ctypes.data_as(C.POINTER(C.c_int32)), None, N,
                                                     hp.ctypes.data_as(C.POINTER(C.c_float)), hb.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == -1, case
        assert (hp == POISON_F).all() and (hb == POISON_I).all(), f"{case}: a refused call wrote outputs"
    else:
        hp, hb = dec.decode_crops_ragged(payload, poffs, index, ioffs, cor.count, hf, h1, N)
        assert np.array_equal(hb, gbits[:6]) and same_bytes(hp.reshape(6, N, bs, ch), got[:6], shape=False), f"{case}: host form"
    assert before.tobytes() == dec.save_streams(slots).tobytes(), f"{case}: the host form changed a stream's state"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. 64-bit addressing
# ---------------------------------------------------------------------------------------------------------------------
def test_files_beyond_4_gib_are_addressed_with_64_bits():
    """A payload buffer of 2^32 + 2^20 bytes, uninitialised but for three files: one below 2^31, one across 2^32, one behind it.
    The bytes between them belong to files nobody crops (the end of one file is the start of the next)."""
    import torch
    amd = _amd()
    r = file_refs(STEREO)
    total = (1 << 32) + (1 << 20)
    try:
        pay = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    except (RuntimeError, MemoryError) as e:
        pytest.skip(f"no {total} bytes of device memory: {e}")
    A, Bf, Cf = r[3], r[4], r[2]                            # 12, 40 and 7 blocks
    a0 = 1001
    b0 = (1 << 32) - Bf.payload.size // 2 - 1
    c0 = b0 + Bf.payload.size
    poffs = np.array([0, a0, a0 + A.payload.size, 1 << 31, b0, c0, c0 + Cf.payload.size, total], np.int64)
    assert a0 + A.payload.size < (1 << 31) and b0 < (1 << 32) < c0 and (np.diff(poffs) < (1 << 31)).all() and poffs[6] + PAD <= total
    cropped = {1: A, 4: Bf, 5: Cf}
    for f, ref in cropped.items():
        pay[int(poffs[f]):int(poffs[f + 1])] = _t(ref.payload)
    caps = [cropped[f].K + 1 if f in cropped else 1 for f in range(7)]
    ioffs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    index = np.zeros(int(ioffs[-1]), INDEX_DTYPE)
    index["RngState"] = 1234567
    for f, ref in cropped.items():
        index[ioffs[f]:ioffs[f + 1]] = ref.row()
    blocks = np.array([cropped[f].K if f in cropped else 0 for f in range(7)], np.int32)
    d = dict(pay=pay, poffs=_t(poffs), idx=_t(index.view(np.int32)), ioffs=_t(ioffs), cnt=_t(blocks))
    mid = (1 << 32) - b0                                    # the byte of the straddling file that lies at address 2^32 of the buffer
    across = int(np.searchsorted(Bf.offs, mid, "right")) - 1
    assert 2 <= across < Bf.K - 2 and Bf.offs[across] < mid <= Bf.offs[across + 1]
    table = [(1, 0), (4, 0), (5, 0), (4, 17), (4, 36), (5, 3), (1, 9), (4, across - 2)]      # (the last row's blocks lie on both sides of 2^32)
    files, first = [f for f, _ in table], [k for _, k in table]
    dec = amd.BatchDecoder(8, 2, 2048, N + 1)
    got, gbits = _ragged_dev(dec, None, d, files, first, N)
    dec.close()
    for i, (f, k) in enumerate(table):
        want, wbits = cropped[f].expected_pcm(k, N)
        assert np.array_equal(gbits[i], wbits) and same_bytes(got[i], want, shape=False), f"row {i}: file {f} (bytes {poffs[f]} ..) from block {k}"
        assert (wbits > 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ragged index
# ---------------------------------------------------------------------------------------------------------------------
SENT = (0x5A5A5A5A, 0xA5A5A5A5)


def _index_dev(dec, payload, poffs, index, ioffs):
    """ulcx_index_packed_ragged_dev -> (index, counts) as numpy; the counts start poisoned"""
    import torch
    F = len(poffs) - 1
    d_pay, d_po, d_idx, d_io = _t(payload), _t(poffs, np.int64), _t(index.view(np.int32)), _t(ioffs, np.int64)
    cnt = torch.full((F,), POISON_I, dtype=torch.int32, device="cuda:0")
    dec.index_packed_ragged_dev(F, d_pay.data_ptr(), d_pay.numel(), d_po.data_ptr(), d_idx.data_ptr(), index.size, d_io.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    return d_idx.cpu().numpy().view(INDEX_DTYPE).reshape(-1), cnt.cpu().numpy()


def test_ragged_index_rows_capacities_sentinels_and_a_damaged_file():
    """Seven files and, between every two, a file whose payload offsets fall (the payloads lie in the buffer in descending
    order: file g starts in front of file g - 1), so that it gets no entry and its row can hold sentinels; two sentinels in
    front of the first row and behind the last.  Capacities: more than the file's blocks (the fill), exactly blocks + 1, fewer
    than its blocks, 1 and 0; one file is damaged and stops the walk where the oracle stops."""
    amd = _amd()
    r = file_refs(STEREO)
    bs, ch = STEREO
    hurt = damaged(r[4].payload, r[4].payload.size, 14)     # (a seed of tests/test_gpu_seek.py's that stops the oracle's walk)
    wbits, woffs, wseeds, inside = oracle_walk(hurt, hurt.size, ch, bs, 44)
    assert inside and 0 < len(wbits) < 40
    # (payload, capacity, blocks expected, expected offsets, expected generator states)
    plan = [(r[0].payload, 4, 1, r[0].offs, r[0].seeds), (r[1].payload, 1, 0, r[1].offs, r[1].seeds), (r[2].payload, 4, 3, r[2].offs, r[2].seeds),
            (r[3].payload, 13, 12, r[3].offs, r[3].seeds), (r[4].payload, 45, 40, r[4].offs, r[4].seeds), (r[1].payload, 0, 0, None, None),
            (hurt, 45, len(wbits), woffs, wseeds)]
    G = len(plan)
    sizes = [p[0].size for p in plan]
    starts = np.cumsum([0] + sizes[::-1])[:-1][::-1] + 3    # file g at starts[g]: descending
    total = int(sum(sizes)) + 3 + PAD
    payload = np.zeros(total, np.uint8)
    poffs, ioffs, real = [], [2], []
    for g, (pay, cap, _, _, _) in enumerate(plan):
        payload[starts[g]:starts[g] + pay.size] = pay
        poffs += [starts[g], starts[g] + pay.size]         # file 2g is [start, end); file 2g + 1 is [end of g, start of g + 1): it falls
        real.append(len(ioffs) - 1)
        ioffs.append(ioffs[-1] + cap)
        if g < G - 1:
            ioffs.append(ioffs[-1] + 2)
    poffs, ioffs = np.array(poffs, np.int64), np.array(ioffs, np.int64)
    F = len(poffs) - 1
    assert F == 2 * G - 1 and len(ioffs) == F + 1 and all(poffs[f + 1] < poffs[f] for f in range(1, F, 2))
    index = np.zeros(int(ioffs[-1]) + 2, INDEX_DTYPE)
    index["ByteOffs"], index["RngState"] = SENT
    one = amd.BatchDecoder(1, ch, bs, 2)
    got, count = _index_dev(one, payload, poffs, index, ioffs)
    want = index.copy()
    for g, (pay, cap, nblk, offs, seeds) in enumerate(plan):
        f = real[g]
        assert count[f] == nblk, f"file {f} (capacity {cap}): {count[f]} blocks, the oracle walks {nblk}"
        if cap > 0:
            row = np.zeros(cap, INDEX_DTYPE)
            row["ByteOffs"] = -1
            row["ByteOffs"][:nblk + 1] = offs[:nblk + 1]
            row["RngState"][:nblk + 1] = seeds[:nblk + 1]
            want[ioffs[f]:ioffs[f + 1]] = row
        assert np.array_equal(got[ioffs[f]:ioffs[f + 1]], want[ioffs[f]:ioffs[f + 1]]), f"file {f} (capacity {cap}): the row differs from the oracle's walk"
        if cap >= 2:                                       # ... and from ulcx_index_packed_rows_dev of that file alone (maxBlocks >= 1)
            alone = np.zeros((1, pay.size + PAD), np.uint8)
            alone[0, :pay.size] = pay
            arow, acnt = one.index_packed_rows(alone, np.array([pay.size], np.int32), cap - 1)
            assert acnt[0] == count[f] and np.array_equal(arow[0], got[ioffs[f]:ioffs[f + 1]]), f"file {f}: ulcx_index_packed_rows_dev of it alone differs"
    for f in range(1, F, 2):
        assert count[f] == 0, f"file {f} has falling offsets and {count[f]} blocks"
    assert np.array_equal(got, want), "an entry outside the rows was written"
    assert (got[:2] == want[:2]).all() and (got[-2:] == want[-2:]).all()
    # the host form: the same table when its offsets are in order, a refusal for these
    with pytest.raises(amd.UlcError, match=r"\(-1\)"):
        one.index_packed_ragged(payload, poffs, ioffs, index=index.copy())
    one.close()


def test_a_one_stream_decoder_indexes_seventy_files():
    """More than one wave, the last one partial; the device form and the host form; rows of blocks + 1 entries."""
    amd = _amd()
    r = file_refs(STEREO)
    cor = Corpus([r[i % 5] for i in range(70)])
    index = np.zeros(cor.ridx.size, INDEX_DTYPE)
    index["ByteOffs"], index["RngState"] = SENT
    one = amd.BatchDecoder(1, 2, 2048, 2)
    got, count = _index_dev(one, cor.rpay, cor.poffs, index, cor.ioffs)
    hidx, hcnt = one.index_packed_ragged(cor.rpay, cor.poffs, cor.ioffs)
    one.close()
    assert np.array_equal(count, cor.count), np.flatnonzero(count != cor.count)
    bad = np.flatnonzero(got != cor.ridx)
    assert bad.size == 0, f"entries {bad[:8]} differ from the oracle's"
    assert np.array_equal(hcnt, count) and np.array_equal(hidx, got)


# ---------------------------------------------------------------------------------------------------------------------
# 7. corpus.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stored", [(1, 3), ()], ids=["two-with-ulx", "none-with-ulx"])
def test_ragged_crop_corpus_equals_the_strided_one_and_is_smaller(stored):
    import torch
    import corpus
    amd = _amd()
    r = file_refs(STEREO)
    bs, ch = STEREO
    both = [corpus.CropCorpus(ch, bs), corpus.CropCorpus(ch, bs, layout="ragged")]
    for cc in both:
        for f, ref in enumerate(r):
            ulc = struct.pack("<IHHIIHHI", 0x32434C55, bs, 0, ref.K, 44100, ch, 0, 24) + ref.payload.tobytes()
            ulx = amd.ulx_pack(ref.row(), ref.K, bs, ch, ref.payload.size) if f in stored else None
            assert cc.add_file(ulc, ulx) == f
        cc.freeze("cuda:0")
    strided, ragged = both
    cor = _corpus(STEREO)
    assert np.array_equal(ragged.d_index_blocks.cpu().numpy(), cor.count)
    assert np.array_equal(ragged.d_index.cpu().numpy().view(INDEX_DTYPE).reshape(-1), cor.ridx), "the frozen index is not the oracle's"
    assert np.array_equal(ragged.d_payload_offs.cpu().numpy(), cor.poffs) and np.array_equal(ragged.d_index_offs.cpu().numpy(), cor.ioffs)
    assert ragged.device_bytes() < strided.device_bytes(), (ragged.device_bytes(), strided.device_bytes())
    assert ragged.device_bytes() == cor.rpay.size + 8 * cor.ridx.size + 2 * 8 * 6 + 4 * 5
    rows = [x for x in ROWS if x[1] <= FILE_BLOCKS[x[0]]]
    files, first, count = [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows]
    dec = amd.BatchDecoder(16, ch, bs, N + 1)
    for pcm16 in (False, True):
        for cnt in (count, None):
            sp, sb = strided.crops(dec, files, first, N, count=cnt, pcm16=pcm16)
            rp, rb = ragged.crops(dec, torch.tensor(files, dtype=torch.int32, device="cuda:0"), first, N, count=cnt, pcm16=pcm16)
            torch.cuda.synchronize()
            assert tuple(rp.shape) == (len(rows), N * bs, ch) and rp.is_cuda and rp.dtype == sp.dtype
            assert torch.equal(rb, sb) and same_bytes(rp.cpu().numpy(), sp.cpu().numpy(), shape=False), (pcm16, cnt)
            if not pcm16:
                want, wbits = cor.expected_pcm(files, first, N, cnt)
                _assert_rows(rp.cpu().numpy().reshape(len(rows), N, bs, ch), rb.cpu().numpy(), want, wbits, files, first, "CropCorpus(layout='ragged').crops")
    dec.close()
