"""Low-rate sample crops on the GPU (include/ulc_amd_lowrate.h: ulcx_decode_crops_lowrate_*): row i of a call is nSamples samples
from sample d_start[i] of the stream of file d_file[i] reduced by D = 1 << lgD, written channels-first.  Every comparison is bit for
bit (uint32 / int16 views) against the referee of tests/lowrate_testlib.py - the oracle's block loop around the oracle's inverse
transform at BlockSize / D on the low bins of the oracle's coefficients - never against this library's own full-rate output."""
import numpy as np
import pytest

from ulc_testlib import same_bytes
from gpu_testlib import amd as _amd, word
import guarded_buffers as gb
import lowrate_testlib as LT
from lowrate_testlib import POISON_F, POISON_I, blocks_of, low_case

pytestmark = pytest.mark.gpu


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _device_rows(dec, lc, files, start, n_samples, length=None, pcm16=False, ragged=False, lgD=None):
    """ulcx_decode_crops_lowrate[_ragged]_dev(_pcm16) on poisoned outputs -> (pcm [n][ch][n_samples], bits [n][nB]) as numpy."""
    import torch
    cor = lc.cor
    d = cor.to_device()
    n = len(files)
    lgD = lc.lgD if lgD is None else lgD
    d_file, d_start = _t(files, np.int32), _t(start, np.int64)
    d_len = _t(length, np.int32) if length is not None else None
    pcm = torch.full((n, cor.ch, n_samples), POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
    bits = torch.full((n, blocks_of(lc.bs >> lgD, n_samples)), POISON_I, dtype=torch.int32, device="cuda:0")
    rows = (n, d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr() if d_len is not None else 0, n_samples, lgD, pcm.data_ptr(), bits.data_ptr())
    if ragged:
        dec.decode_crops_lowrate_ragged_dev(cor.F, d["rpay"].data_ptr(), cor.rpay.size, d["poffs"].data_ptr(), d["ridx"].data_ptr(), cor.ridx.size,
                                            d["ioffs"].data_ptr(), d["cnt"].data_ptr(), *rows, pcm16=pcm16)
    else:
        dec.decode_crops_lowrate_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride,
                                     d["cnt"].data_ptr(), *rows, pcm16=pcm16)
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), bits.cpu().numpy()


def _check_rows(lc, table, n_samples, pcm, bits, what, pcm16=False, rows=None):
    for i in (range(len(table)) if rows is None else rows):
        f, st, ln = table[i]
        want, wb = lc.expected_row(int(f), int(st), n_samples, ln, pcm16)
        where = f"{lc.name}, {what}: row {i} (file {f} from reduced sample {st}, length {ln})"
        assert np.array_equal(bits[i], wb), f"{where}: bits {bits[i]} vs the oracle's {wb}"
        if not same_bytes(pcm[i], want):
            bad = np.argwhere(pcm[i].view(np.uint16 if pcm16 else np.uint32) != want.view(np.uint16 if pcm16 else np.uint32))
            err = np.abs(pcm[i].astype(np.float64) - want.astype(np.float64)).max()
            raise AssertionError(f"{where}: {len(bad)} of {want.size} samples differ from the referee's, first at (channel, t) = {bad[0].tolist()}, "
                                 f"last at {bad[-1].tolist()}, largest difference {err:g}")


def _cols(table):
    return [f for f, _, _ in table], [s for _, s, _ in table], [l for _, _, l in table]


# ---------------------------------------------------------------------------------------------------------------------
# 1. every geometry and ratio: the row table through every form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LT.CASES))
def test_lowrate_rows_equal_the_referees(name):
    amd = _amd()
    lc = low_case(name)
    cor, bsr = lc.cor, lc.bsr
    n_samples = 3 * bsr + 1
    table = lc.row_table(n_samples)
    assert 20 <= len(table) <= 70
    files, start, length = _cols(table)
    assert amd.lowrate_block(lc.bs, lc.lgD) == bsr
    dec = amd.BatchDecoder(len(table), lc.ch, lc.bs, blocks_of(bsr, n_samples) + 1)
    for pcm16 in (False, True):
        pcm, bits = _device_rows(dec, lc, files, start, n_samples, length, pcm16)
        _check_rows(lc, table, n_samples, pcm, bits, "pcm16" if pcm16 else "float", pcm16)
        live = [i for i in range(len(table)) if (bits[i] > 0).any()]
        assert len(live) >= 10 and sum((pcm[i] != 0).any() for i in live) >= 8, (name, len(live))
    pcm, bits = _device_rows(dec, lc, files, start, n_samples, length, ragged=True)
    _check_rows(lc, table, n_samples, pcm, bits, "ragged")
    pcm, bits = _device_rows(dec, lc, files, start, n_samples, None)                    # NULL d_len: every row takes nSamples
    _check_rows(lc, [(f, s, n_samples) for f, s, _ in table], n_samples, pcm, bits, "without lengths")
    # the host forms, on the rows they do not refuse
    ok = [i for i, (f, s, l) in enumerate(table) if 0 <= f < cor.F and 0 <= s <= cor.K[f] * bsr]
    sub = [table[i] for i in ok]
    hf, hs, hl = _cols(sub)
    hp, hb = dec.decode_crops_lowrate(cor.host, cor.nbytes, cor.index, cor.count, hf, hs, n_samples, lc.lgD, length=hl)
    _check_rows(lc, sub, n_samples, hp, hb, "host form")
    r = cor.ragged()
    hp, hb = dec.decode_crops_lowrate_ragged(r["payload"], r["poffs"], r["index"], r["ioffs"], r["blocks"], hf, hs, n_samples, lc.lgD, length=hl)
    _check_rows(lc, sub, n_samples, hp, hb, "ragged host form")
    dec.close()


def test_one_sample_per_row():
    amd = _amd()
    lc = low_case("2048x2/2")
    table = [(f, s, 1) for f, s, _ in lc.row_table(1)]
    files, start, length = _cols(table)
    dec = amd.BatchDecoder(len(table), lc.ch, lc.bs, 2)
    for pcm16 in (False, True):
        pcm, bits = _device_rows(dec, lc, files, start, 1, None, pcm16)
        assert pcm.shape == (len(table), lc.ch, 1) and bits.shape == (len(table), 1)
        _check_rows(lc, table, 1, pcm, bits, "one sample", pcm16)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. launch plans: few long rows (the even cut), more rows than the device holds at once
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2048x2/2", "8192x2/2"])
def test_few_long_rows_take_the_even_cut(name):
    amd = _amd()
    lc = low_case(name)
    bsr = lc.bsr
    nblk = min(30, lc.cor.K[0] - 2)
    n_samples = (nblk - 1) * bsr + 1
    assert blocks_of(bsr, n_samples) == nblk
    table = [(0, bsr + 1001 % bsr, n_samples), (0, 0, n_samples)]
    files, start, length = _cols(table)
    dec = amd.BatchDecoder(2, lc.ch, lc.bs, nblk + 1)
    for pcm16 in (False, True):
        pcm, bits = _device_rows(dec, lc, files, start, n_samples, None, pcm16)
        grid, whole, _ = dec.last_cut()
        assert grid > 2 and whole == 0, (grid, whole)              # more workgroups than rows: every row is in pieces
        _check_rows(lc, table, n_samples, pcm, bits, "even cut", pcm16)
        assert (bits > 0).all()
    dec.close()


def test_more_rows_than_workgroup_slots():
    amd = _amd()
    lc = low_case("2048x2/4")
    bsr, cor = lc.bsr, lc.cor
    n_samples = 4 * bsr + 2
    nB = blocks_of(bsr, n_samples)
    probe = amd.BatchDecoder(8, lc.ch, lc.bs, nB + 1)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0
    n = 2 * resident + resident * 2 // 3                         # (the reduced kernel holds at least as many workgroups as the full one)
    rng = np.random.default_rng(33)
    files = rng.integers(0, cor.F - 1, n).astype(np.int32)
    start = np.array([rng.integers(0, cor.K[f] * bsr - n_samples) for f in files], np.int64)
    start[0], start[n - 1] = 0, cor.K[files[n - 1]] * bsr - n_samples // 2
    table = [(int(f), int(s), n_samples) for f, s in zip(files, start)]
    dec = amd.BatchDecoder(n, lc.ch, lc.bs, nB + 1)
    pcm, bits = _device_rows(dec, lc, files, start, n_samples)
    grid, whole, _ = dec.last_cut()
    assert grid > 0, (grid, whole)
    pick = sorted(set([0, 1, resident - 1, resident, resident + 1, 2 * resident, n - 2, n - 1] + rng.integers(0, n, 24).tolist()))
    _check_rows(lc, table, n_samples, pcm, bits, f"{n} rows over {grid} workgroups ({whole} whole)", rows=pick)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. lgD 0 is the sample-crop call; the identity with spectra -> low bins -> synthesis at BS'
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2048x2/2", "1024x6/4"])
def test_ratio_one_is_the_sample_crop_call(name):
    import torch
    amd = _amd()
    lc = low_case(name)
    cor, bs = lc.cor, lc.bs
    n_samples = 2 * bs + 3
    table = lc.row_table(n_samples)
    files, start, length = [f for f, _, _ in table], [s * (1 << lc.lgD) + 1 for _, s, _ in table], [l for _, _, l in table]
    dec = amd.BatchDecoder(len(table), lc.ch, bs, blocks_of(bs, n_samples) + 1)
    d = cor.to_device()
    for pcm16 in (False, True):
        got, gbits = _device_rows(dec, lc, files, start, n_samples, length, pcm16, lgD=0)
        pcm = torch.full(got.shape, POISON_I if pcm16 else POISON_F, dtype=torch.int16 if pcm16 else torch.float32, device="cuda:0")
        bits = torch.full(gbits.shape, POISON_I, dtype=torch.int32, device="cuda:0")
        d_file, d_start, d_len = _t(files, np.int32), _t(start, np.int64), _t(length, np.int32)
        dec.decode_crops_samples_dev(cor.F, d["pay"].data_ptr(), cor.host.shape[1], d["nb"].data_ptr(), d["idx"].data_ptr(), cor.istride, d["cnt"].data_ptr(),
                                     len(table), d_file.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n_samples, pcm.data_ptr(), bits.data_ptr(), pcm16=pcm16)
        torch.cuda.synchronize()
        assert same_bytes(got, pcm.cpu().numpy()) and np.array_equal(gbits, bits.cpu().numpy())
        assert (gbits > 0).any() and (got != 0).any()
    dec.close()


@pytest.mark.parametrize("name", ["2048x2/4", "2048x3/2", "codes 2048x2/2"])
def test_identity_with_spectra_low_bins_and_synthesis_at_the_reduced_size(name):
    amd = _amd()
    lc = low_case(name)
    cor, bs, bsr, ch = lc.cor, lc.bs, lc.bsr, lc.ch
    N = 4
    n_samples = N * bsr
    firsts = [(0, 1), (0, 5), (0, cor.K[0] - 2), (1, 3), (cor.F - 1, lc.dead_at - 2), (1, cor.K[1] - N)]
    files, first = [f for f, _ in firsts], [k for _, k in firsts]
    dec = amd.BatchDecoder(len(firsts), ch, bs, N + 2)
    got, gbits = _device_rows(dec, lc, files, [k * bsr for k in first], n_samples)
    coef, wc, sbits = dec.decode_crops_spectra(cor.host, cor.nbytes, cor.index, cor.count, files, [k - 1 for k in first], N + 1)
    low = np.zeros((len(firsts), ch, N + 1, bsr), np.float32)
    for i in range(len(firsts)):
        for k in range(N + 1):
            at = at_r = 0
            for S in (amd.window_subblocks(bs, int(wc[i, k])) if wc[i, k] else []):
                low[i, :, k, at_r:at_r + (S >> lc.lgD)] = coef[i, :, k, at:at + (S >> lc.lgD)]
                at += S; at_r += S >> lc.lgD
    small = amd.BatchDecoder(len(firsts), ch, bsr, N + 2)
    pcm, live = small.synth_spectra(low, wc, flags=amd.SYNTH_WARM)
    assert same_bytes(got, pcm.reshape(got.shape)), name
    assert np.array_equal(gbits[:, :N] > 0, live > 0) and np.array_equal(gbits[:, :N], sbits[:, 1:])
    assert (live[[0, 1, 3, 5]] > 0).all() and (live[2] > 0).sum() == 2 and (live[4] > 0).sum() == 2      # (row 2 ends with its file, row 4 at the dead block)
    small.close(); dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the object's state; the caller's buffers
# ---------------------------------------------------------------------------------------------------------------------
def test_lowrate_crops_between_two_halves_of_a_packed_decode():
    """A decoder half-way through decode_packed of its own streams: low-rate calls at every ratio, under both launch plans, change no
    byte of any slot's saved record, and the packed decode goes on as the oracle's uninterrupted one."""
    amd = _amd()
    B = 8
    cases = [low_case(n) for n in ("2048x2/2", "2048x2/4", "2048x2/8")]
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
    for lc in cases:
        for n_blk in (3, 22):
            n_samples = (n_blk - 1) * lc.bsr + 1
            table = [(k % 2, k * lc.bsr + 17 * k, n_samples) for k in range(B if n_blk == 22 else 3)]
            files, start, _ = _cols(table)
            pcm, bits = _device_rows(dec, lc, files, start, n_samples)
            _check_rows(lc, table, n_samples, pcm, bits, f"{len(table)} rows x {n_samples}")
    assert before.tobytes() == dec.save_streams(slots).tobytes(), "a low-rate call changed a stream's state"
    packed(6, 6, "behind the low-rate calls")
    dec.close()


G_B = 8


def _arena(lc, n, n_samples, pcm16):
    import torch
    cor = lc.cor
    F, stride = cor.host.shape
    esz = 2 if pcm16 else 4
    nB = blocks_of(lc.bsr, n_samples)
    specs = [dict(name="d_payload", nbytes=F * stride, align=1, role="in", guard=F * stride, row=stride),
             word("d_payloadBytes", F, "in"),
             dict(name="d_index", nbytes=8 * F * cor.istride, align=4, role="in", guard=8 * F * cor.istride, row=8, rows_per_stream=cor.istride),
             word("d_indexBlocks", F, "in"), word("d_file", n, "in", G_B),
             dict(name="d_start", nbytes=8 * n, align=8, role="in", guard=8 * G_B, row=8), word("d_len", n, "in", G_B),
             dict(name="d_pcm", nbytes=n * lc.ch * n_samples * esz, align=esz, role="out", guard=G_B * lc.ch * n_samples * esz, row=n_samples * esz,
                  rows_per_stream=lc.ch),
             word("d_bits", n * nB, "out", G_B * (nB + 1), nB)]
    a = gb.build(torch.device("cuda", 0), specs)
    a.load("d_payload", cor.host); a.load("d_payloadBytes", cor.nbytes); a.load("d_index", cor.index); a.load("d_indexBlocks", cor.count)
    return a


@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
@pytest.mark.parametrize("name", ["2048x2/2", "1024x6/4"])
def test_lowrate_entries_on_poisoned_guarded_buffers(name, pcm16):
    """Every element of both outputs is written over the poison, nothing lands in a guard, no input changes; d_pcm sits at an odd
    multiple of its element's size and a plane has an odd number of samples.  Then the refusals that need an object: nothing is
    touched by any of them."""
    import torch
    amd = _amd()
    lc = low_case(name)
    cor, bsr = lc.cor, lc.bsr
    n_samples = 2 * bsr + 1
    z = cor.F - 1
    table = [(0, 0, n_samples), (0, 3 * bsr + 1, bsr), (0, cor.K[0] * bsr - 100, n_samples), (z, (lc.dead_at - 1) * bsr - 1, n_samples), (0, 5 * bsr, 1),
             (cor.F + 2, 5, n_samples)]
    files, start, length = _cols(table)
    n = len(table)
    a = _arena(lc, n, n_samples, pcm16)
    assert a.ptr("d_pcm") % (4 if pcm16 else 8) != 0
    a.load("d_file", np.array(files, np.int32)); a.load("d_start", np.array(start, np.int64)); a.load("d_len", np.array(length, np.int32))
    dec = amd.BatchDecoder(G_B, lc.ch, lc.bs, blocks_of(bsr, n_samples) + 1)

    def call(lgD, ns=n_samples, off=None):
        p = lambda nm: a.ptr(nm) + (off or {}).get(nm, 0)
        dec.decode_crops_lowrate_dev(cor.F, p("d_payload"), cor.host.shape[1], p("d_payloadBytes"), p("d_index"), cor.istride, p("d_indexBlocks"),
                                     n, p("d_file"), p("d_start"), p("d_len"), ns, lgD, p("d_pcm"), p("d_bits"), pcm16=pcm16)

    who = "ulcx_decode_crops_lowrate_dev" + ("_pcm16" if pcm16 else "")
    too_far = next(l for l in range(5) if l > 3 or (lc.bs >> l) < 256)
    for bad, kw in ((dict(lgD=-1), "lgD -1"), (dict(lgD=4), "lgD 4"), (dict(lgD=too_far), f"lgD {too_far}"), (dict(lgD=lc.lgD, ns=8 * bsr), "nSamples"),
                    (dict(lgD=lc.lgD, off={"d_start": 4}), "d_start"), (dict(lgD=lc.lgD, off={"d_pcm": 1}), "d_pcm")):
        with pytest.raises(amd.UlcError, match=r"\(-1\)"):
            call(**bad)
        msg = amd.lib().ulcx_last_error().decode()
        assert msg.startswith(who + ":") and kw in msg, msg
    torch.cuda.synchronize()
    a.check()
    assert a.fetch("d_pcm").tobytes() == gb.pattern(a.regions["d_pcm"].off, a.regions["d_pcm"].nbytes).tobytes(), "a refused call wrote samples"
    assert a.fetch("d_bits").tobytes() == gb.pattern(a.regions["d_bits"].off, a.regions["d_bits"].nbytes).tobytes(), "a refused call wrote sizes"
    call(lc.lgD)
    torch.cuda.synchronize()
    a.check()
    got = a.fetch("d_pcm", np.int16 if pcm16 else np.float32).reshape(n, lc.ch, n_samples)
    gbits = a.fetch("d_bits", np.int32).reshape(n, -1)
    _check_rows(lc, table, n_samples, got, gbits, "guarded call", pcm16)
    dec.close()


def test_host_forms_refuse_what_the_device_forms_cannot():
    amd = _amd()
    lc = low_case("2048x2/2")
    cor, bsr = lc.cor, lc.bsr
    n_samples = bsr + 1
    dec = amd.BatchDecoder(4, lc.ch, lc.bs, blocks_of(bsr, n_samples) + 1)
    K0 = cor.K[0]
    r = cor.ragged()
    for hf, hs, hl, kw in (([0, -1], [0, 0], None, "row 1 "), ([0, cor.F], [0, 0], None, "row 1 "), ([0, 0], [0, -1], None, "row 1 "),
                           ([0, 0], [0, K0 * bsr + 1], None, "row 1 "), ([0, 0], [0, 0], [1, -1], "row 1 ")):
        for ragged in (False, True):
            with pytest.raises(amd.UlcError, match=r"\(-1\)"):
                if ragged:
                    dec.decode_crops_lowrate_ragged(r["payload"], r["poffs"], r["index"], r["ioffs"], r["blocks"], hf, hs, n_samples, lc.lgD, length=hl)
                else:
                    dec.decode_crops_lowrate(cor.host, cor.nbytes, cor.index, cor.count, hf, hs, n_samples, lc.lgD, length=hl)
            msg = amd.lib().ulcx_last_error().decode()
            assert msg.startswith("ulcx_decode_crops_lowrate" + ("_ragged" if ragged else "") + "_host: " + kw), msg
    # a start of exactly indexBlocks * BS' is a row of zeros, not a refusal; one reduced block short of the FULL stream's end is refused
    hp, hb = dec.decode_crops_lowrate(cor.host, cor.nbytes, cor.index, cor.count, [0, 0], [K0 * bsr, 3], n_samples, lc.lgD)
    assert (hp[0] == 0).all() and (hb[0] == 0).all() and (hb[1] > 0).all()
    _check_rows(lc, [(0, K0 * bsr, n_samples), (0, 3, n_samples)], n_samples, hp, hb, "host form")
    with pytest.raises(amd.UlcError, match=r"\(-1\)"):
        dec.decode_crops_lowrate(cor.host, cor.nbytes, cor.index, cor.count, [0], [K0 * lc.bs - 5], n_samples, lc.lgD)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. through corpus.py
# ---------------------------------------------------------------------------------------------------------------------
def test_crop_corpus_sample_crops_at_low_rates():
    import struct
    import torch
    import corpus
    amd = _amd()
    lc = low_case("2048x2/4")
    cor = lc.cor
    F = cor.F - 1                                               # (the clean files: add_file indexes what it is given)
    ccs = {}
    for layout in ("strided", "ragged"):
        cc = corpus.CropCorpus(cor.ch, cor.bs, layout=layout)
        for f in range(F):
            pay = cor.host[f, :cor.nbytes[f]].tobytes()
            ulc = struct.pack("<IHHIIHHI", 0x32434C55, cor.bs, 0, cor.K[f], 44100, cor.ch, 0, 24) + pay
            assert cc.add_file(ulc, None) == f
        ccs[layout] = cc.freeze("cuda:0")
    n_samples = 3 * lc.bsr + 5
    table = [(f, s, l) for f, s, l in lc.row_table(n_samples) if 0 <= f < F and s >= 0]
    files, start, length = _cols(table)
    dec = amd.BatchDecoder(len(table), cor.ch, cor.bs, amd.crop_blocks(lc.bsr, n_samples) + 1)
    for pcm16 in (False, True):
        for layout, cc in ccs.items():
            pcm, bits = cc.sample_crops(dec, files, torch.tensor(start, dtype=torch.int64, device="cuda:0"), n_samples, length=length, pcm16=pcm16, lowrate=lc.lgD)
            assert tuple(pcm.shape) == (len(table), cor.ch, n_samples) and pcm.is_cuda
            torch.cuda.synchronize()
            _check_rows(lc, table, n_samples, pcm.cpu().numpy(), bits.cpu().numpy(), f"CropCorpus({layout}).sample_crops(lowrate={lc.lgD})", pcm16)
    with pytest.raises(ValueError):
        ccs["strided"].sample_crops(dec, files, start, n_samples, lowrate=4)
    dec.close()
