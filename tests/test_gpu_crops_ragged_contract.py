"""The caller-buffer contract (include/ulc_amd.h, "Caller buffers") of the ragged-corpus calls - ulcx_decode_crops_ragged_dev /
_dev_pcm16 / _host and ulcx_index_packed_ragged_dev: every buffer of a call carved from one poisoned arena between guards
(tests/guarded_buffers.py), each pointer misaligned in turn, and follow-up work on the call's stream without a
synchronisation.  The reference is the oracle's sequential decode and its walk (tests/ragged_testlib.py)."""
import ctypes as C
import functools
import numpy as np
import pytest

from gpu_testlib import amd as _amd, dev as _dev, word
import guarded_buffers as gb
from ulc_testlib import to_pcm16, same_bytes
from corpus_testlib import INDEX_DTYPE, Corpus
from ragged_testlib import file_refs

pytestmark = pytest.mark.gpu
A_PCM, A_PCM16, A_OFFS, A_WORD, A_BYTE = 16, 8, 8, 4, 1    # the header's ALIGNMENT table
BS, CH, B, N, MAXK = 2048, 2, 8, 3, 5                      # a decoder of 8 streams, 5 blocks per call; calls of 3
SENT = (0x5A5A5A5A, 0xA5A5A5A5)


@functools.lru_cache(maxsize=None)
def _corpus():
    """The files of 2, 7, 12 and 40 blocks with NO byte behind the last payload: the buffer ends with the longest file's last block."""
    r = file_refs((BS, CH))
    cor = Corpus([r[1], r[2], r[3], r[4]])
    cor.rpay = np.ascontiguousarray(cor.rpay[:cor.poffs[-1]])
    return cor


F = 4
K = (2, 7, 12, 40)


def _offs(name):
    return dict(name=name, nbytes=8 * (F + 1), align=A_OFFS, role="in", guard=8 * (F + 1), row=8)


def _arena(n, pcm16, with_count=True, device="gpu"):
    cor = _corpus()
    row = BS * CH * (2 if pcm16 else 4)
    specs = [dict(name="d_payload", nbytes=cor.rpay.size, align=A_BYTE, role="in", guard=cor.rpay.size, row=cor.rpay.size),
             _offs("d_payloadOffs"),
             dict(name="d_index", nbytes=8 * cor.ridx.size, align=A_WORD, role="in", guard=8 * cor.ridx.size, row=8),
             _offs("d_indexOffs"), word("d_indexBlocks", F, "in"), word("d_file", n, "in", B), word("d_first", n, "in", B)]
    if with_count:
        specs.append(word("d_count", n, "in", B))
    specs += [dict(name="d_pcm", nbytes=n * N * row, align=A_PCM16 if pcm16 else A_PCM, role="out", guard=B * MAXK * row, row=row, rows_per_stream=N),
              word("d_bits", n * N, "out", B * MAXK, N)]
    a = gb.build(_dev() if device == "gpu" else None, specs)
    a.load("d_payload", cor.rpay); a.load("d_payloadOffs", cor.poffs); a.load("d_index", cor.ridx); a.load("d_indexOffs", cor.ioffs)
    a.load("d_indexBlocks", cor.count)
    return a


def _call(dec, a, n, pcm16, stream=0, off=None):
    """off: {name: bytes} added to a pointer (the misalignment cases)"""
    cor = _corpus()
    p = lambda name: (a.ptr(name) + (off or {}).get(name, 0)) if name in a.regions else 0
    dec.decode_crops_ragged_dev(F, p("d_payload"), cor.rpay.size, p("d_payloadOffs"), p("d_index"), cor.ridx.size, p("d_indexOffs"), p("d_indexBlocks"),
                                n, p("d_file"), p("d_first"), p("d_count"), N, p("d_pcm"), p("d_bits"), stream=stream, pcm16=pcm16)


def _check(a, n, files, first, count, pcm16, what):
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, N, BS, CH)
    gbits = a.fetch("d_bits", np.int32).reshape(n, N)
    want, wb = _corpus().expected_pcm(files, first, N, count)
    want = to_pcm16(want) if pcm16 else want
    for i in range(n):
        assert np.array_equal(gbits[i], wb[i]), f"{what}: row {i} (file {files[i]} from block {first[i]}): bits {gbits[i]} != {wb[i]}"
        assert same_bytes(got[i], want[i], shape=False), f"{what}: row {i} (file {files[i]} from block {first[i]}): samples differ"


# row 1 ends with the buffer's last byte; row 2 runs past its file's end; rows 4 and 5: a bad start, a bad file
ROWS = ([3, 3, 0, 1, 2, F], [0, 38, 1, 3, K[2] + 1, 0], [3, 3, 3, 1, 3, 3])


@pytest.mark.parametrize("with_count", [True, False], ids=["count", "no-count"])
@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_ragged_crop_entries_on_poisoned_guarded_buffers(pcm16, with_count):
    """Outputs are written in full over the poison (zeros and 0 bits where a row has no block), nothing lands in a guard, no
    input changes - the file at the payload buffer's very end is read up to its last block."""
    import torch
    amd = _amd()
    files, first, count = ROWS
    n = len(files)
    a = _arena(n, pcm16, with_count)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32))
    if with_count:
        a.load("d_count", np.array(count, np.int32))
    dec = amd.BatchDecoder(B, CH, BS, MAXK)
    _call(dec, a, n, pcm16)
    torch.cuda.synchronize()
    dec.close()
    a.check()
    _check(a, n, files, first, count if with_count else None, pcm16, "guarded call")


def test_ragged_host_form_on_poisoned_guarded_host_buffers():
    amd = _amd()
    cor = _corpus()
    files, first, count = ROWS[0][:4], ROWS[1][:4], ROWS[2][:4]                 # (the host form refuses the two bad rows)
    n = len(files)
    a = _arena(n, False, device="host")
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32)); a.load("d_count", np.array(count, np.int32))
    dec = amd.BatchDecoder(B, CH, BS, MAXK)
    p = lambda name, t: C.cast(a.ptr(name), C.POINTER(t))
    rc = amd.lib().ulcx_decode_crops_ragged_host(dec.h, F, p("d_payload", C.c_uint8), cor.rpay.size, p("d_payloadOffs", C.c_int64), a.ptr("d_index"),
                                                 cor.ridx.size, p("d_indexOffs", C.c_int64), p("d_indexBlocks", C.c_int32), n, p("d_file", C.c_int32),
                                                 p("d_first", C.c_int32), p("d_count", C.c_int32), N, p("d_pcm", C.c_float), p("d_bits", C.c_int32))
    dec.close()
    assert rc == 0, amd.lib().ulcx_last_error().decode()
    a.check()
    _check(a, n, files, first, count, False, "guarded host call")


def test_ragged_index_on_poisoned_guarded_buffers():
    """d_index is in and out: the rows are written in full, the sentinel entries in front of the first row and behind the last
    stay; d_nBlocks is written in full."""
    import torch
    amd = _amd()
    cor = _corpus()
    ioffs = cor.ioffs + 3
    index = np.zeros(cor.ridx.size + 6, INDEX_DTYPE)
    index["ByteOffs"], index["RngState"] = SENT
    specs = [dict(name="d_payload", nbytes=cor.rpay.size, align=A_BYTE, role="in", guard=cor.rpay.size, row=cor.rpay.size),
             _offs("d_payloadOffs"),
             dict(name="d_index", nbytes=8 * index.size, align=A_WORD, role="inout", guard=8 * index.size, row=8),
             _offs("d_indexOffs"), word("d_nBlocks", F, "out")]
    a = gb.build(_dev(), specs)
    a.load("d_payload", cor.rpay); a.load("d_payloadOffs", cor.poffs); a.load("d_index", index); a.load("d_indexOffs", ioffs)
    dec = amd.BatchDecoder(1, CH, BS, 2)
    dec.index_packed_ragged_dev(F, a.ptr("d_payload"), cor.rpay.size, a.ptr("d_payloadOffs"), a.ptr("d_index"), index.size, a.ptr("d_indexOffs"),
                                a.ptr("d_nBlocks"))
    torch.cuda.synchronize()
    a.check()
    want = index.copy()
    want[3:-3] = cor.ridx
    assert np.array_equal(a.fetch("d_nBlocks", np.int32), cor.count)
    assert np.array_equal(a.fetch("d_index").view(INDEX_DTYPE), want)
    # each pointer misaligned in turn: refused, nothing written
    a.repoison("d_nBlocks"); a.load("d_index", index)
    for name, by in (("d_payloadOffs", 4), ("d_indexOffs", 4), ("d_index", 2), ("d_nBlocks", 2)):
        p = lambda k: a.ptr(k) + (by if k == name else 0)
        with pytest.raises(amd.UlcError, match=r"\(-1\).*" + name + r".*not aligned"):
            dec.index_packed_ragged_dev(F, p("d_payload"), cor.rpay.size, p("d_payloadOffs"), p("d_index"), index.size, p("d_indexOffs"), p("d_nBlocks"))
    torch.cuda.synchronize()
    dec.close()
    a.check()
    assert np.array_equal(a.fetch("d_index").view(INDEX_DTYPE), index), "a refused call wrote entries"
    assert a.fetch("d_nBlocks").tobytes() == gb.pattern(a.regions["d_nBlocks"].off, a.regions["d_nBlocks"].nbytes).tobytes(), "a refused call wrote counts"


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_misaligned_ragged_crop_pointers_are_refused_and_nothing_is_touched(pcm16):
    """Each pointer in turn off the alignment the header states - the two offset tables at 4 bytes off their 8: ULCX_ERR_ARG
    before any device work - the outputs keep their poison, the guards hold, every slot's saved record (a decoder in the middle
    of a packed decode) is byte-equal, and the next valid call is correct."""
    import torch
    amd = _amd()
    files, first, count = ROWS
    n = len(files)
    cor = _corpus()
    host, nb = cor.host, cor.nbytes
    a = _arena(n, pcm16)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32)); a.load("d_count", np.array(count, np.int32))
    dec = amd.BatchDecoder(B, CH, BS, MAXK)
    pick = np.arange(B) % 2 + 2                             # the files of 12 and 40 blocks
    dec.decode_packed(host[pick], nb[pick], 2)
    before = dec.save_streams(list(range(B)))
    offs = [("d_payloadOffs", 4), ("d_indexOffs", 4), ("d_payloadOffs", 1), ("d_index", 2), ("d_indexBlocks", 1), ("d_file", 2), ("d_first", 2), ("d_count", 3),
            ("d_pcm", 4 if pcm16 else 8), ("d_pcm", 2 if pcm16 else 4), ("d_bits", 2)]
    for name, by in offs:
        with pytest.raises(amd.UlcError, match=r"\(-1\).*" + name + r".*not aligned"):
            _call(dec, a, n, pcm16, off={name: by})
    torch.cuda.synchronize()
    a.check()
    assert a.fetch("d_pcm").tobytes() == gb.pattern(a.regions["d_pcm"].off, a.regions["d_pcm"].nbytes).tobytes(), "a refused call wrote samples"
    assert a.fetch("d_bits").tobytes() == gb.pattern(a.regions["d_bits"].off, a.regions["d_bits"].nbytes).tobytes(), "a refused call wrote sizes"
    assert before.tobytes() == dec.save_streams(list(range(B))).tobytes(), "a refused call changed a stream's state"
    _call(dec, a, n, pcm16)                                 # (an odd payload address is no misalignment: the region is carved at one)
    torch.cuda.synchronize()
    a.check()
    _check(a, n, files, first, count, pcm16, "valid call behind the refused ones")
    assert before.tobytes() == dec.save_streams(list(range(B))).tobytes(), "the crop call changed a stream's state"
    pcm, bits = dec.decode_packed(host[pick], nb[pick], 2)  # the packed decode goes on
    want, wb = cor.expected_pcm(list(pick), [2] * B, 2)
    for s in range(B):
        assert np.array_equal(bits[s], wb[s]) and same_bytes(pcm[s].reshape(2, BS, CH), want[s], shape=False), f"stream {s} behind the crop call"
    dec.close()


def test_work_behind_a_ragged_crop_call_on_its_stream_is_ordered():
    """Two crop calls back to back on a torch.cuda.Stream, nothing waits for the host in between: rows copied into the carved
    regions, the call, outputs copied away, then rows AND outputs overwritten with poison - all on that stream.  Both calls'
    saved outputs must equal the oracle.  (A pass cannot prove there is no race; a failure is a finding.)"""
    import torch
    amd = _amd()
    dev = _dev()
    n = 5
    calls = [([3, 0, 3, 1, 2], [0, 0, 38, 3, 1], [3, 3, 3, 1, 2]), ([2, 2, 1, 0, 3], [3, 0, 4, 1, 20], [3, 0, 3, 3, 3])]
    a = _arena(n, False)
    st = torch.cuda.Stream(device=dev)
    ins = ("d_file", "d_first", "d_count")
    outs = ("d_pcm", "d_bits")
    src = [{k: torch.from_numpy(np.array(v, np.int32)).to(dev).view(torch.uint8) for k, v in zip(ins, c)} for c in calls]
    poison = {k: a.poison_of(k) for k in ins + outs}
    saved = [{k: torch.empty_like(a.view(k)) for k in outs} for _ in calls]
    dec = amd.BatchDecoder(B, CH, BS, MAXK)
    torch.cuda.synchronize()                                # everything above is in place; from here on only the stream orders
    with torch.cuda.stream(st):
        for c in range(len(calls)):
            for k in ins:
                a.view(k).copy_(src[c][k], non_blocking=True)
            _call(dec, a, n, False, stream=st.cuda_stream)
            for k in outs:
                saved[c][k].copy_(a.view(k), non_blocking=True)
            for k in ins + outs:
                a.view(k).copy_(poison[k], non_blocking=True)
    st.synchronize()
    for k in ins:
        a.expect(k, poison[k].cpu().numpy())
    a.check()
    dec.close()
    for c, (files, first, count) in enumerate(calls):
        got = saved[c]["d_pcm"].cpu().numpy().view(np.float32).reshape(n, N, BS, CH)
        gbits = saved[c]["d_bits"].cpu().numpy().view(np.int32).reshape(n, N)
        want, wb = _corpus().expected_pcm(files, first, N, count)
        assert np.array_equal(gbits, wb), f"call {c}: bits {gbits.tolist()} != {wb.tolist()}"
        assert same_bytes(got, want, shape=False), f"call {c}: samples differ"
