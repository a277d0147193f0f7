"""The caller-buffer contract (include/ulc_amd.h, "Caller buffers") of ulcx_decode_crops_dev / _dev_pcm16: every buffer of the
call carved from one poisoned arena between guards (tests/guarded_buffers.py), each pointer misaligned in turn, and follow-up
work on the call's stream without a synchronisation.  The reference is the oracle's sequential decode (tests/seek_testlib.py)."""
import functools
import numpy as np
import pytest

from ulc_testlib import to_pcm16, same_bytes
from gpu_testlib import amd as _amd, dev as _dev, word
import guarded_buffers as gb
from seek_testlib import expected_range
from corpus_testlib import Corpus, oracle_file

pytestmark = pytest.mark.gpu
A_PCM, A_PCM16, A_WORD, A_BYTE = 16, 8, 4, 1               # the header's ALIGNMENT table
BS, CH, L, F, B, N, MAXK = 2048, 2, 6, 4, 8, 3, 5          # four files of 6 blocks; a decoder of 8 streams, 5 blocks per call; calls of 3


@functools.lru_cache(maxsize=None)
def _corpus():
    """Four oracle streams packed with no byte behind the longest (the payload buffer ends with the last file's stride), their
    index from the oracle's block sizes and generator states, and the oracle's decode of each."""
    cor = Corpus([oracle_file(BS, CH, q, sid, 11, L) for q, sid in ((50.0, 3), (50.0, 4), (35.0, 5), (65.0, 6))])
    tight = (int(cor.nbytes.max()) + 15) & ~15
    return np.ascontiguousarray(cor.host[:, :tight]), cor.nbytes, cor.index, cor.count, [(f.pcm, f.obits) for f in cor.files]


def _arena(n, pcm16, with_count=True):
    host, nb, index, count, _ = _corpus()
    stride = host.shape[1]
    row = BS * CH * (2 if pcm16 else 4)
    specs = [dict(name="d_payload", nbytes=F * stride, align=A_BYTE, role="in", guard=F * stride, row=stride),
             word("d_payloadBytes", F, "in"),
             dict(name="d_index", nbytes=8 * F * (L + 1), align=A_WORD, role="in", guard=8 * F * (L + 1), row=8, rows_per_stream=L + 1),
             word("d_indexBlocks", F, "in"), word("d_file", n, "in", B), word("d_first", n, "in", B)]
    if with_count:
        specs.append(word("d_count", n, "in", B))
    specs += [dict(name="d_pcm", nbytes=n * N * row, align=A_PCM16 if pcm16 else A_PCM, role="out", guard=B * MAXK * row, row=row, rows_per_stream=N),
              word("d_bits", n * N, "out", B * MAXK, N)]
    a = gb.build(_dev(), specs)
    a.load("d_payload", host); a.load("d_payloadBytes", nb); a.load("d_index", index); a.load("d_indexBlocks", count)
    return a, stride


def _call(dec, a, stride, n, pcm16, stream=0, off=None):
    """off: {name: bytes} added to a pointer (the misalignment cases)"""
    p = lambda name: (a.ptr(name) + (off or {}).get(name, 0)) if name in a.regions else 0
    dec.decode_crops_dev(F, p("d_payload"), stride, p("d_payloadBytes"), p("d_index"), L + 1, p("d_indexBlocks"), n, p("d_file"), p("d_first"),
                         p("d_count"), N, p("d_pcm"), p("d_bits"), stream=stream, pcm16=pcm16)


def _expected(files, first, count, pcm16):
    refs = _corpus()[4]
    out, ob = [], []
    for i, f in enumerate(files):
        ok = 0 <= f < F and 0 <= first[i] <= L
        want, wb = expected_range(refs[f][0], refs[f][1], int(first[i]), N) if ok else (np.zeros((N, BS, CH), np.float32), np.zeros(N, np.int32))
        if count is not None:
            m = max(0, min(N, int(count[i])))
            want[m:] = 0; wb[m:] = 0
        out.append(to_pcm16(want) if pcm16 else want); ob.append(wb)
    return np.stack(out), np.stack(ob)


def _check(a, n, files, first, count, pcm16, what):
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, N, BS, CH)
    gbits = a.fetch("d_bits", np.int32).reshape(n, N)
    want, wb = _expected(files, first, count, pcm16)
    for i in range(n):
        assert np.array_equal(gbits[i], wb[i]), f"{what}: row {i} (file {files[i]} from block {first[i]}): bits {gbits[i]} != {wb[i]}"
        assert same_bytes(got[i], want[i], shape=False), f"{what}: row {i} (file {files[i]} from block {first[i]}): samples differ"


ROWS = ([3, 0, 3, 1, 2, F], [0, 2, 5, 3, L + 1, 0], [3, 3, 3, 1, 3, 3])      # row 2 runs past its end; rows 4 and 5: a bad start, a bad file


@pytest.mark.parametrize("with_count", [True, False], ids=["count", "no-count"])
@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_crop_entries_on_poisoned_guarded_buffers(pcm16, with_count):
    """Outputs are written in full over the poison (zeros and 0 bits where a row has no block), nothing lands in a guard, no
    input changes - the file at the payload buffer's very end (file 3) is read by two rows."""
    import torch
    amd = _amd()
    files, first, count = ROWS
    n = len(files)
    a, stride = _arena(n, pcm16, with_count)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32))
    if with_count:
        a.load("d_count", np.array(count, np.int32))
    dec = amd.BatchDecoder(B, CH, BS, MAXK)
    _call(dec, a, stride, n, pcm16)
    torch.cuda.synchronize()
    dec.close()
    a.check()
    _check(a, n, files, first, count if with_count else None, pcm16, "guarded call")


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_misaligned_crop_pointers_are_refused_and_nothing_is_touched(pcm16):
    """Each pointer in turn off the alignment the header states: ULCX_ERR_ARG before any device work - the outputs keep their
    poison, the guards hold, every slot's saved record (a decoder in the middle of a packed decode) is byte-equal, and the next
    valid call is correct."""
    import torch
    amd = _amd()
    files, first, count = ROWS
    n = len(files)
    host, nb, _, _, refs = _corpus()
    a, stride = _arena(n, pcm16)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32)); a.load("d_count", np.array(count, np.int32))
    dec = amd.BatchDecoder(B, CH, BS, MAXK)
    pick = np.arange(B) % F
    dec.decode_packed(host[pick], nb[pick], 2)
    before = dec.save_streams(list(range(B)))
    offs = [("d_payloadBytes", 2), ("d_index", 2), ("d_indexBlocks", 1), ("d_file", 2), ("d_first", 2), ("d_count", 3),
            ("d_pcm", 4 if pcm16 else 8), ("d_pcm", 2 if pcm16 else 4), ("d_bits", 2)]
    for name, by in offs:
        with pytest.raises(amd.UlcError, match=r"\(-1\).*" + name + r".*not aligned"):
            _call(dec, a, stride, n, pcm16, off={name: by})
    torch.cuda.synchronize()
    a.check()
    assert a.fetch("d_pcm").tobytes() == gb.pattern(a.regions["d_pcm"].off, a.regions["d_pcm"].nbytes).tobytes(), "a refused call wrote samples"
    assert a.fetch("d_bits").tobytes() == gb.pattern(a.regions["d_bits"].off, a.regions["d_bits"].nbytes).tobytes(), "a refused call wrote sizes"
    assert before.tobytes() == dec.save_streams(list(range(B))).tobytes(), "a refused call changed a stream's state"
    _call(dec, a, stride, n, pcm16)                         # (an odd payload address is no misalignment: the region is carved at one)
    torch.cuda.synchronize()
    a.check()
    _check(a, n, files, first, count, pcm16, "valid call behind the refused ones")
    assert before.tobytes() == dec.save_streams(list(range(B))).tobytes(), "the crop call changed a stream's state"
    pcm, bits = dec.decode_packed(host[pick], nb[pick], 2)  # the packed decode goes on
    for s in range(B):
        want, wb = expected_range(refs[pick[s]][0], refs[pick[s]][1], 2, 2)
        assert np.array_equal(bits[s], wb) and same_bytes(pcm[s].reshape(2, BS, CH), want, shape=False), f"stream {s} behind the crop call"
    dec.close()


def test_work_behind_a_crop_call_on_its_stream_is_ordered():
    """Two crop calls back to back on a torch.cuda.Stream, nothing waits for the host in between: rows copied into the carved
    regions, the call, outputs copied away, then rows AND outputs overwritten with poison - all on that stream.  Both calls'
    saved outputs must equal the oracle.  (A pass cannot prove there is no race; a failure is a finding.)"""
    import torch
    amd = _amd()
    dev = _dev()
    n = 5
    calls = [([3, 0, 3, 1, 2], [0, 2, 5, 3, 1], [3, 3, 3, 1, 2]), ([2, 2, 1, 0, 3], [3, 0, 4, 1, 2], [3, 0, 3, 3, 3])]
    a, stride = _arena(n, False)
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
            _call(dec, a, stride, n, False, stream=st.cuda_stream)
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
        want, wb = _expected(files, first, count, False)
        assert np.array_equal(gbits, wb), f"call {c}: bits {gbits.tolist()} != {wb.tolist()}"
        assert same_bytes(got, want, shape=False), f"call {c}: samples differ"
