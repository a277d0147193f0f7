"""Mid and side crops on the GPU (include/ulc_amd_part.h: ulcx_decode_crops_part_*): row i of a call is nSamples samples from sample
d_start[i] of the stream of file d_file[i] reduced by 1 << lgD, one plane per channel pair - coded channel 2 j + part as the decoder
holds it in front of its un-mix.  Every comparison is bit for bit (uint32 / int16 views) against tests/part_testlib.py - the oracle's
block loop as a ONE-channel decoder around the oracle's inverse transform, per coded channel - never against this library's own
stereo output.  Mid and side run on the same rows in one test: a side taken from the generator state at the block's start, or a mid
where the side belongs, differs from the referee's wherever the block's mid channel drew noise (the census of test_part_capi.py)."""
import numpy as np
import pytest

from ulc_testlib import same_bytes
from gpu_testlib import amd as _amd, word
import guarded_buffers as gb
import part_testlib as PT
from part_testlib import POISON_F, POISON_I, MID, SIDE, blocks_of, part_case, part_channels, parts_of

pytestmark = pytest.mark.gpu


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _prepare(pc, part, files, start, n_samples, length=None, pcm16=False, lgD=None):
    """The rows and the poisoned outputs of one call on the device -> the call's tail of arguments and (pcm, bits, the rows' tensors)."""
    import torch
    n = len(files)
    lgD = pc.lgD if lgD is None else lgD
    d_file, d_start = _t(files, np.int32), _t(start, np.int64)
    d_len = _t(length, np.int32) if length is not None else None
    pcm = torch.full((n, part_channels(pc.cor.ch, part), n_samples), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full((n, blocks_of(pc.bs >> lgD, n_samples)), POISON_I, dtype=torch.int32, device="cuda:0")
    rows = (n, d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr() if d_len is not None else 0, n_samples, lgD, part, pcm.data_ptr(), bits.data_ptr())
    return rows, (pcm, bits, d_file, d_start, d_len)


def _enqueue(dec, pc, rows, pcm16=False, ragged=False):
    """ulcx_decode_crops_part[_ragged]_dev(_pcm16) on torch's current stream."""
    import torch
    cor = pc.cor
    d = cor.to_device()
    stream = torch.cuda.current_stream().cuda_stream
    if ragged:
        dec.decode_crops_part_ragged_dev(cor.F, d["rpay"].data_ptr(), cor.rpay.size, d["poffs"].data_ptr(), d["ridx"].data_ptr(), cor.ridx.size,
                                         d["ioffs"].data_ptr(), d["cnt"].data_ptr(), *rows, stream=stream, pcm16=pcm16)
    else:
        dec.decode_crops_part_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride,
                                  d["cnt"].data_ptr(), *rows, stream=stream, pcm16=pcm16)


def _device_rows(dec, pc, part, files, start, n_samples, length=None, pcm16=False, ragged=False, lgD=None):
    """One call on poisoned outputs -> (pcm [n][nOut][n_samples], bits [n][nB]) as numpy."""
    import torch
    rows, keep = _prepare(pc, part, files, start, n_samples, length, pcm16, lgD)
    torch.cuda.synchronize()
    _enqueue(dec, pc, rows, pcm16, ragged)
    torch.cuda.synchronize()
    return keep[0].cpu().numpy(), keep[1].cpu().numpy()


def _check_rows(pc, part, table, n_samples, pcm, bits, what, pcm16=False, rows=None):
    assert pcm.shape == (len(table), part_channels(pc.ch, part), n_samples), (pcm.shape, what)
    for i in (range(len(table)) if rows is None else rows):
        f, st, ln = table[i]
        want, wb = pc.expected_row(int(f), int(st), n_samples, ln, part, pcm16)
        where = f"{pc.name} {'side' if part else 'mid'}, {what}: row {i} (file {f} from reduced sample {st}, length {ln})"
        assert np.array_equal(bits[i], wb), f"{where}: bits {bits[i]} vs the oracle's {wb}"
        if not same_bytes(pcm[i], want):
            bad = np.argwhere(pcm[i].view(np.uint16 if pcm16 else np.uint32) != want.view(np.uint16 if pcm16 else np.uint32))
            err = np.abs(pcm[i].astype(np.float64) - want.astype(np.float64)).max()
            raise AssertionError(f"{where}: {len(bad)} of {want.size} samples differ from the referee's, first at (plane, t) = {bad[0].tolist()}, "
                                 f"last at {bad[-1].tolist()}, largest difference {err:g}")


def _cols(table):
    return [f for f, _, _ in table], [s for _, s, _ in table], [l for _, _, l in table]


# ---------------------------------------------------------------------------------------------------------------------
# 1. every case: the row table, mid and side, through every form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PT.CASES))
def test_part_rows_equal_the_referees(name):
    amd = _amd()
    pc = part_case(name)
    cor, bsr = pc.cor, pc.bsr
    n_samples = 3 * bsr + 1
    table = pc.row_table(n_samples)
    files, start, length = _cols(table)
    dec = amd.BatchDecoder(len(table), pc.ch, pc.bs, blocks_of(bsr, n_samples) + 1)
    ok = [i for i, (f, s, l) in enumerate(table) if 0 <= f < cor.F and 0 <= s <= cor.K[f] * bsr]       # the rows the host forms do not refuse
    sub = [table[i] for i in ok]
    hf, hs, hl = _cols(sub)
    r = cor.ragged()
    floats = {}
    for part in parts_of(pc.ch):
        assert amd.part_channels(pc.ch, part) == part_channels(pc.ch, part) > 0
        for pcm16 in (False, True):
            pcm, bits = _device_rows(dec, pc, part, files, start, n_samples, length, pcm16)
            _check_rows(pc, part, table, n_samples, pcm, bits, "pcm16" if pcm16 else "float", pcm16)
            live = [i for i in range(len(table)) if (bits[i] > 0).any()]
            assert len(live) >= 10 and sum((pcm[i] != 0).any() for i in live) >= 8, (name, part, len(live))
            if not pcm16:
                floats[part] = pcm
        pcm, bits = _device_rows(dec, pc, part, files, start, n_samples, length, ragged=True)
        _check_rows(pc, part, table, n_samples, pcm, bits, "ragged")
        pcm, bits = _device_rows(dec, pc, part, files, start, n_samples, length, pcm16=True, ragged=True)
        _check_rows(pc, part, table, n_samples, pcm, bits, "ragged pcm16", True)
        pcm, bits = _device_rows(dec, pc, part, files, start, n_samples, None)                 # NULL d_len: every row takes nSamples
        _check_rows(pc, part, [(f, s, n_samples) for f, s, _ in table], n_samples, pcm, bits, "without lengths")
        hp, hb = dec.decode_crops_part(cor.host, cor.nbytes, cor.index, cor.count, hf, hs, n_samples, part, pc.lgD, length=hl)
        _check_rows(pc, part, sub, n_samples, hp, hb, "host form")
        hp, hb = dec.decode_crops_part_ragged(r["payload"], r["poffs"], r["index"], r["ioffs"], r["blocks"], hf, hs, n_samples, part, pc.lgD, length=hl)
        _check_rows(pc, part, sub, n_samples, hp, hb, "ragged host form")
    if SIDE in floats:                                         # the two parts are different signals: neither call handed out the other's channel
        n_pairs = part_channels(pc.ch, SIDE)
        assert not same_bytes(floats[MID][:, :n_pairs], floats[SIDE]), name
    dec.close()


def test_one_sample_per_row():
    amd = _amd()
    pc = part_case("2048x2/1")
    table = [(f, s, 1) for f, s, _ in pc.row_table(1)]
    files, start, _ = _cols(table)
    dec = amd.BatchDecoder(len(table), pc.ch, pc.bs, 2)
    for part in (MID, SIDE):
        for pcm16 in (False, True):
            pcm, bits = _device_rows(dec, pc, part, files, start, 1, None, pcm16)
            assert bits.shape == (len(table), 1)
            _check_rows(pc, part, table, 1, pcm, bits, "one sample", pcm16)
    dec.close()


@pytest.mark.parametrize("name", ["2048x2/0", "8192x2/1"])
def test_few_long_rows_one_workgroup_each(name):
    """Four rows over 30 blocks of the case's longest file: the call is not cut (include/ulc_amd_part.h, LAUNCH) and says so through
    ulcx_decoder_last_cut."""
    amd = _amd()
    pc = part_case(name)
    bsr = pc.bsr
    nblk = min(30, pc.cor.K[0] - 2)
    n_samples = (nblk - 1) * bsr + 1
    assert blocks_of(bsr, n_samples) == nblk
    table = [(0, bsr + 1001 % bsr, n_samples), (0, 0, n_samples), (0, 2 * bsr - 1, n_samples), (0, bsr, n_samples)]
    files, start, _ = _cols(table)
    dec = amd.BatchDecoder(4, pc.ch, pc.bs, nblk + 1)
    for part in (MID, SIDE):
        for pcm16 in (False, True):
            pcm, bits = _device_rows(dec, pc, part, files, start, n_samples, None, pcm16)
            assert dec.last_cut()[:2] == (0, 0)
            _check_rows(pc, part, table, n_samples, pcm, bits, "long rows", pcm16)
            assert (bits > 0).all()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the identities: spectra -> channel plane -> low bins -> synthesis on a one-channel decoder; mid of mono is the low-rate call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2048x2/1", "2048x3/1", "codes 2048x2/1"])
def test_identity_with_spectra_one_plane_low_bins_and_a_one_channel_synthesis(name):
    amd = _amd()
    pc = part_case(name)
    cor, bs, bsr, ch = pc.cor, pc.bs, pc.bsr, pc.ch
    N = 4
    n_samples = N * bsr
    firsts = [(0, 1), (0, 5), (0, cor.K[0] - 2), (1, 3), (cor.F - 1, pc.dead_at - 2), (1, cor.K[1] - N)]
    files, first = [f for f, _ in firsts], [k for _, k in firsts]
    dec = amd.BatchDecoder(len(firsts), ch, bs, N + 2)
    coef, wc, sbits = dec.decode_crops_spectra(cor.host, cor.nbytes, cor.index, cor.count, files, [k - 1 for k in first], N + 1)      # no ULCX_SPECTRA_LR
    small = amd.BatchDecoder(len(firsts), 1, bsr, N + 2)
    for part in parts_of(ch):
        got, gbits = _device_rows(dec, pc, part, files, [k * bsr for k in first], n_samples)
        for j in range(part_channels(ch, part)):
            c = 2 * j + part
            low = np.zeros((len(firsts), 1, N + 1, bsr), np.float32)
            for i in range(len(firsts)):
                for k in range(N + 1):
                    at = at_r = 0
                    for S in (amd.window_subblocks(bs, int(wc[i, k])) if wc[i, k] else []):
                        low[i, 0, k, at_r:at_r + (S >> pc.lgD)] = coef[i, c, k, at:at + (S >> pc.lgD)]
                        at += S; at_r += S >> pc.lgD
            pcm, live = small.synth_spectra(low, wc, flags=amd.SYNTH_WARM)
            assert same_bytes(got[:, j], pcm.reshape(len(firsts), n_samples)), (name, part, j)
            assert np.array_equal(gbits[:, :N] > 0, live > 0) and np.array_equal(gbits[:, :N], sbits[:, 1:])
        assert (gbits[[0, 1, 3, 5], :N] > 0).all() and (gbits[2] > 0).sum() == 2 and (gbits[4] > 0).sum() == 2    # (row 2 ends with its file, row 4 at the dead block)
    small.close(); dec.close()


@pytest.mark.parametrize("name,lgD", [("512x1/0", 0), ("512x1/0", 1), ("codes 1024x1/0", 0), ("codes 1024x1/0", 2)])
def test_mid_of_a_mono_corpus_is_the_lowrate_call(name, lgD):
    import torch
    amd = _amd()
    pc = part_case(name)
    cor, bsr = pc.cor, pc.bs >> lgD
    n_samples = 2 * bsr + 3
    table = pc.row_table(n_samples)
    files, start, length = [f for f, _, _ in table], [s >> lgD for _, s, _ in table], [l for _, _, l in table]
    dec = amd.BatchDecoder(len(table), 1, pc.bs, blocks_of(bsr, n_samples) + 1)
    d = cor.to_device()
    for pcm16 in (False, True):
        got, gbits = _device_rows(dec, pc, MID, files, start, n_samples, length, pcm16, lgD=lgD)
        pcm = torch.full(got.shape, POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
        bits = torch.full(gbits.shape, POISON_I, dtype=torch.int32, device="cuda:0")
        d_file, d_start, d_len = _t(files, np.int32), _t(start, np.int64), _t(length, np.int32)
        dec.decode_crops_lowrate_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                     len(table), d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n_samples, lgD, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
        torch.cuda.synchronize()
        assert same_bytes(got, pcm.cpu().numpy()) and np.array_equal(gbits, bits.cpu().numpy())
        assert (gbits > 0).any() and (got != 0).any()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the object's state and the stream's order
# ---------------------------------------------------------------------------------------------------------------------
def test_part_crops_between_two_halves_of_a_packed_decode():
    """A decoder half-way through decode_packed of its own streams: part calls of both parts at every ratio - each ratio's first call
    on an object that has already streamed - change no byte of any slot's saved record, and the packed decode goes on as the oracle's
    uninterrupted one."""
    amd = _amd()
    B = 8
    cases = [part_case(n) for n in ("2048x2/0", "2048x2/1", "2048x2/3")]
    cor, bs, ch = cases[0].cor, 2048, 2
    pick = np.arange(B) % 2
    host, nbytes = np.ascontiguousarray(cor.host[pick]), cor.nbytes[pick]
    dec = amd.BatchDecoder(B, ch, bs, 24)
    slots = list(range(B))

    def packed(at, n, what):
        pcm, bits = dec.decode_packed(host, nbytes, n)
        for s in range(B):
            want, wb = cor.files[pick[s]].expected_pcm(at, n)
            assert np.array_equal(bits[s], wb) and same_bytes(np.asarray(pcm[s], np.float32).reshape(want.shape), want), f"{what}: stream {s}, blocks {at}.."

    packed(0, 6, "first half")
    before = dec.save_streams(slots)
    for pc in cases:
        for part in (SIDE, MID):
            for n_blk in (3, 22):
                n_samples = (n_blk - 1) * pc.bsr + 1
                table = [(k % 2, k * pc.bsr + 17 * k, n_samples) for k in range(B if n_blk == 22 else 3)]
                files, start, _ = _cols(table)
                pcm, bits = _device_rows(dec, pc, part, files, start, n_samples)
                _check_rows(pc, part, table, n_samples, pcm, bits, f"{len(table)} rows x {n_samples}")
        assert before.tobytes() == dec.save_streams(slots).tobytes(), "a part call changed a stream's state"
    packed(6, 6, "behind the part calls")
    dec.close()


def test_part_calls_behind_filler_work_on_a_stream_of_their_own():
    """On a non-default stream, behind torch work that is still running when the first call returns, and without the host waiting in
    between: side, mid, then the stereo sample-crop call into buffers of their own."""
    import torch
    amd = _amd()
    pc = part_case("2048x2/1")
    cor, bsr = pc.cor, pc.bsr
    n_samples = 2 * bsr + 5
    table = pc.row_table(n_samples)
    files, start, length = _cols(table)
    dec = amd.BatchDecoder(len(table), pc.ch, pc.bs, blocks_of(bsr, n_samples) + 1)
    _device_rows(dec, pc, MID, files, start, n_samples, length)                 # (the ratio's tables are built: the calls below only enqueue)
    st = torch.cuda.Stream()
    x = torch.randn(2048, 2048, device="cuda:0")
    y = torch.empty_like(x)
    r_side, side = _prepare(pc, SIDE, files, start, n_samples, length)
    r_mid, mid = _prepare(pc, MID, files, start, n_samples, length)
    r_low, low = _prepare(pc, SIDE, files, start, n_samples, length, pcm16=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for _ in range(40):
            torch.mm(x, x, out=y)
        ev = torch.cuda.Event()
        ev.record()
        _enqueue(dec, pc, r_side)
        started = ev.query()
        _enqueue(dec, pc, r_mid)
        _enqueue(dec, pc, r_low, pcm16=True, ragged=True)
    st.synchronize()
    assert not started, "the device had passed the filler when the first call returned - the calls ran behind an idle stream"
    _check_rows(pc, SIDE, table, n_samples, side[0].cpu().numpy(), side[1].cpu().numpy(), "side behind the filler")
    _check_rows(pc, MID, table, n_samples, mid[0].cpu().numpy(), mid[1].cpu().numpy(), "mid behind side")
    _check_rows(pc, SIDE, table, n_samples, low[0].cpu().numpy(), low[1].cpu().numpy(), "ragged pcm16 side behind mid", True)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the caller's buffers; refusals
# ---------------------------------------------------------------------------------------------------------------------
G_B = 8


def _arena(pc, part, n, n_samples, pcm16):
    import torch
    cor = pc.cor
    F, stride = cor.host.shape
    esz = 2 if pcm16 else 4
    nB = blocks_of(pc.bsr, n_samples)
    n_out = part_channels(pc.ch, part)
    specs = [dict(name="d_payload", nbytes=F * stride, align=1, role="in", guard=F * stride, row=stride),
             word("d_payloadBytes", F, "in"),
             dict(name="d_index", nbytes=8 * F * cor.istride, align=4, role="in", guard=8 * F * cor.istride, row=8, rows_per_stream=cor.istride),
             word("d_indexBlocks", F, "in"), word("d_file", n, "in", G_B),
             dict(name="d_start", nbytes=8 * n, align=8, role="in", guard=8 * G_B, row=8), word("d_len", n, "in", G_B),
             # (the guard behind the samples is longer than all the planes a stereo call would write: a second plane would land in it)
             dict(name="d_pcm", nbytes=n * n_out * n_samples * esz, align=esz, role="out", guard=G_B * pc.ch * n_samples * esz, row=n_samples * esz,
                  rows_per_stream=n_out),
             word("d_bits", n * nB, "out", G_B * (nB + 1), nB)]
    a = gb.build(torch.device("cuda", 0), specs)
    a.load("d_payload", cor.host); a.load("d_payloadBytes", cor.nbytes); a.load("d_index", cor.index); a.load("d_indexBlocks", cor.count)
    return a


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
@pytest.mark.parametrize("name,part", [("2048x2/1", MID), ("2048x2/1", SIDE), ("2048x3/1", MID), ("1024x6/2", SIDE)])
def test_part_entries_on_poisoned_guarded_buffers(name, part, pcm16):
    """Every element of both outputs - [n][nOut][nSamples] and [n][nB] - is written over the poison, nothing lands in a guard (where
    the planes of the other part would lie in a stereo call's output), no input changes; d_pcm sits at an odd multiple of its
    element's size and a plane has an odd number of samples.  Then the refusals that need an object: nothing is touched by any."""
    import torch
    amd = _amd()
    pc = part_case(name)
    cor, bsr = pc.cor, pc.bsr
    n_samples = 2 * bsr + 1
    z = cor.F - 1
    table = [(0, 0, n_samples), (0, 3 * bsr + 1, bsr), (0, cor.K[0] * bsr - 100, n_samples), (z, (pc.dead_at - 1) * bsr - 1, n_samples), (0, 5 * bsr, 1),
             (cor.F + 2, 5, n_samples)]
    files, start, length = _cols(table)
    n = len(table)
    a = _arena(pc, part, n, n_samples, pcm16)
    assert a.ptr("d_pcm") % (4 if pcm16 else 8) != 0
    a.load("d_file", np.array(files, np.int32)); a.load("d_start", np.array(start, np.int64)); a.load("d_len", np.array(length, np.int32))
    dec = amd.BatchDecoder(G_B, pc.ch, pc.bs, blocks_of(bsr, n_samples) + 1)

    def call(lgD, part=part, ns=n_samples, off=None):
        p = lambda nm: a.ptr(nm) + (off or {}).get(nm, 0)
        dec.decode_crops_part_dev(cor.F, p("d_payload"), cor.host.shape[1], p("d_payloadBytes"), p("d_index"), cor.istride, p("d_indexBlocks"),
                                  n, p("d_file"), p("d_start"), p("d_len"), ns, lgD, part, p("d_pcm"), p("d_bits"), pcm16=pcm16)

    who = "ulcx_decode_crops_part_dev" + ("_pcm16" if pcm16 else "")
    too_far = next(l for l in range(5) if l > 3 or (pc.bs >> l) < 256)
    for bad, kw in ((dict(lgD=pc.lgD, part=-1), "part -1"), (dict(lgD=pc.lgD, part=2), "part 2"), (dict(lgD=-1), "lgD -1"), (dict(lgD=4), "lgD 4"),
                    (dict(lgD=too_far), f"lgD {too_far}"), (dict(lgD=pc.lgD, ns=8 * bsr), "nSamples"),
                    (dict(lgD=pc.lgD, off={"d_start": 4}), "d_start"), (dict(lgD=pc.lgD, off={"d_pcm": 1}), "d_pcm")):
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            call(**bad)
        msg = amd.lib().ulcx_last_error().decode()
        assert msg.startswith(who + ":") and kw in msg, msg
    torch.cuda.synchronize()
    a.check()
    assert a.fetch("d_pcm").tobytes() == gb.pattern(a.regions["d_pcm"].off, a.regions["d_pcm"].nbytes).tobytes(), "a refused call wrote samples"
    assert a.fetch("d_bits").tobytes() == gb.pattern(a.regions["d_bits"].off, a.regions["d_bits"].nbytes).tobytes(), "a refused call wrote sizes"
    call(pc.lgD)
    torch.cuda.synchronize()
    a.check()
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, part_channels(pc.ch, part), n_samples)
    gbits = a.fetch("d_bits", np.int32).reshape(n, -1)
    _check_rows(pc, part, table, n_samples, got, gbits, "guarded call", pcm16)
    dec.close()


def test_the_side_of_a_mono_corpus_is_refused():
    import torch
    amd = _amd()
    pc = part_case("512x1/0")
    cor = pc.cor
    n_samples = pc.bs + 1
    dec = amd.BatchDecoder(4, 1, pc.bs, blocks_of(pc.bs, n_samples) + 1)
    for ragged in (False, True):
        for pcm16 in (False, True):
            with pytest.raises(amd.UlcError, match=r"\(-1\)"):
                _call_side_of_mono(dec, pc, n_samples, pcm16, ragged)
            msg = amd.lib().ulcx_last_error().decode()
            assert msg.startswith("ulcx_decode_crops_part" + ("_ragged" if ragged else "") + "_dev" + ("_pcm16" if pcm16 else "") + ":") and "part 1" in msg, msg
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            if ragged:
                r = cor.ragged()
                dec.decode_crops_part_ragged(r["payload"], r["poffs"], r["index"], r["ioffs"], r["blocks"], [0], [0], n_samples, SIDE)
            else:
                dec.decode_crops_part(cor.host, cor.nbytes, cor.index, cor.count, [0], [0], n_samples, SIDE)
        assert "part 1" in amd.lib().ulcx_last_error().decode()
    torch.cuda.synchronize()
    dec.close()


def _call_side_of_mono(dec, pc, n_samples, pcm16, ragged):
    """the device forms with part = SIDE on a one-channel object: one plane of poison stands where a plane would go"""
    import torch
    cor = pc.cor
    d = cor.to_device()
    d_file, d_start = _t([0, 0], np.int32), _t([0, 5], np.int64)
    pcm = torch.full((2, 1, n_samples), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full((2, blocks_of(pc.bs, n_samples)), POISON_I, dtype=torch.int32, device="cuda:0")
    rows = (2, d_file.data_ptr(), d_start.data_ptr(), 0, n_samples, 0, SIDE, pcm.data_ptr(), bits.data_ptr())
    try:
        if ragged:
            dec.decode_crops_part_ragged_dev(cor.F, d["rpay"].data_ptr(), cor.rpay.size, d["poffs"].data_ptr(), d["ridx"].data_ptr(), cor.ridx.size,
                                             d["ioffs"].data_ptr(), d["cnt"].data_ptr(), *rows, pcm16=pcm16)
        else:
            dec.decode_crops_part_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride,
                                      d["cnt"].data_ptr(), *rows, pcm16=pcm16)
    finally:
        torch.cuda.synchronize()
        assert (pcm == (POISON_I if pcm16 else POISON_F)).all() and (bits == POISON_I).all(), "a refused call wrote"


def test_host_forms_refuse_what_the_device_forms_cannot():
    amd = _amd()
    pc = part_case("2048x2/1")
    cor, bsr = pc.cor, pc.bsr
    n_samples = bsr + 1
    dec = amd.BatchDecoder(4, pc.ch, pc.bs, blocks_of(bsr, n_samples) + 1)
    K0 = cor.K[0]
    r = cor.ragged()
    for hf, hs, hl, kw in (([0, -1], [0, 0], None, "row 1 "), ([0, cor.F], [0, 0], None, "row 1 "), ([0, 0], [0, -1], None, "row 1 "),
                           ([0, 0], [0, K0 * bsr + 1], None, "row 1 "), ([0, 0], [0, 0], [1, -1], "row 1 ")):
        for ragged in (False, True):
            with pytest.raises(amd.UlcError, match=r"\(-1\)"):
                if ragged:
                    dec.decode_crops_part_ragged(r["payload"], r["poffs"], r["index"], r["ioffs"], r["blocks"], hf, hs, n_samples, SIDE, pc.lgD, length=hl)
                else:
                    dec.decode_crops_part(cor.host, cor.nbytes, cor.index, cor.count, hf, hs, n_samples, SIDE, pc.lgD, length=hl)
            msg = amd.lib().ulcx_last_error().decode()
            assert msg.startswith("ulcx_decode_crops_part" + ("_ragged" if ragged else "") + "_host: " + kw), msg
    hp, hb = dec.decode_crops_part(cor.host, cor.nbytes, cor.index, cor.count, [0, 0], [K0 * bsr, 3], n_samples, SIDE, pc.lgD)
    assert hp.shape == (2, 1, n_samples) and (hp[0] == 0).all() and (hb[0] == 0).all() and (hb[1] > 0).all()
    _check_rows(pc, SIDE, [(0, K0 * bsr, n_samples), (0, 3, n_samples)], n_samples, hp, hb, "host form")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. through corpus.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2048x2/1", "2048x3/1"])
def test_crop_corpus_sample_crops_of_a_part(name):
    import struct
    import torch
    import corpus
    amd = _amd()
    pc = part_case(name)
    cor = pc.cor
    F = cor.F - 1                                               # (the clean files: add_file indexes what it is given)
    ccs = {}
    for layout in ("strided", "ragged"):
        cc = corpus.CropCorpus(cor.ch, cor.bs, layout=layout)
        for f in range(F):
            pay = cor.host[f, :cor.nbytes[f]].tobytes()
            ulc = struct.pack("<IHHIIHHI", 0x32434C55, cor.bs, 0, cor.K[f], 44100, cor.ch, 0, 24) + pay
            assert cc.add_file(ulc, None) == f
        ccs[layout] = cc.freeze("cuda:0")
    n_samples = 3 * pc.bsr + 5
    table = [(f, s, l) for f, s, l in pc.row_table(n_samples) if 0 <= f < F and s >= 0]
    files, start, length = _cols(table)
    dec = amd.BatchDecoder(len(table), cor.ch, cor.bs, amd.crop_blocks(pc.bsr, n_samples) + 1)
    st = torch.cuda.Stream()
    for pcm16 in (False, True):
        for layout, cc in ccs.items():
            for part, word_ in ((MID, "mid"), (SIDE, "side")):
                with torch.cuda.stream(st):                     # torch's current stream, not the null stream
                    pcm, bits = cc.sample_crops(dec, files, torch.tensor(start, dtype=torch.int64, device="cuda:0"), n_samples, length=length, pcm16=pcm16,
                                                lowrate=pc.lgD, part=word_)
                assert tuple(pcm.shape) == (len(table), part_channels(cor.ch, part), n_samples) and pcm.is_cuda
                st.synchronize()
                _check_rows(pc, part, table, n_samples, pcm.cpu().numpy(), bits.cpu().numpy(), f"CropCorpus({layout}).sample_crops(part={word_})", pcm16)
    with pytest.raises(ValueError):
        ccs["strided"].sample_crops(dec, files, start, n_samples, part="left")
    with pytest.raises(ValueError):
        ccs["strided"].sample_crops(dec, files, start, n_samples, lowrate=4, part="mid")
    dec.close()
