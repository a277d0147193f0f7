"""Spectra on the GPU (include/ulc_amd.h section 3: ulcx_decode_crops_spectra_*): the dequantised MDCT coefficients of crop rows.
Every comparison is bit for bit (uint32 views) against the oracle (tests/spectra_testlib.py): orc_decode_stream_coefs run
sequentially over the whole file and sliced, channels-first; LR formed from that in numpy float32; the window codes from each
block's first byte; zeros where a block is not live.  d_bits is additionally compared with what ulcx_decode_crops_dev returns for
the same rows.  The device calls run on poisoned buffers carved between guards (tests/guarded_buffers.py); what the inputs hold -
noise units of several passes, every decimation pattern, the units that fill the LDS - is asserted in tests/test_spectra_capi.py."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd, dev as _dev, word
import guarded_buffers as gb
import spectra_testlib as S
from seek_testlib import geometries, oracle_pcm
import damage_testlib as D

pytestmark = pytest.mark.gpu
GEOMS = sorted(geometries().keys())
N = S.N_BLOCKS
LR = S.SPECTRA_LR


def spectra_dev(dec, lay, ch, bs, files, first, nb, count=None, flags=0):
    """One ulcx_decode_crops_spectra(_ragged)_dev call with every buffer carved from a poisoned arena between guards -> (coef
    [n][ch][nb][bs], wc [n][nb], bits [n][nb]) after the guards and the inputs have been checked.  lay: dict(host, nbytes, index,
    count) of a strided corpus, or dict(payload, poffs, index, ioffs, blocks) of a ragged one."""
    import torch
    n = len(files)
    ragged = "poffs" in lay
    plane = 4 * nb * bs
    specs = [word("d_indexBlocks", len(lay["blocks" if ragged else "count"]), "in"), word("d_file", n, "in"), word("d_first", n, "in")]
    if ragged:
        specs += [dict(name="d_payload", nbytes=lay["payload"].size, align=1, role="in"),
                  dict(name="d_payloadOffs", nbytes=8 * lay["poffs"].size, align=8, role="in"),
                  dict(name="d_index", nbytes=8 * lay["index"].size, align=4, role="in"),
                  dict(name="d_indexOffs", nbytes=8 * lay["ioffs"].size, align=8, role="in")]
    else:
        specs += [dict(name="d_payload", nbytes=lay["host"].size, align=1, role="in", row=lay["host"].shape[1]), word("d_payloadBytes", lay["nbytes"].size, "in"),
                  dict(name="d_index", nbytes=8 * lay["index"].size, align=4, role="in")]
    if count is not None:
        specs.append(word("d_count", n, "in"))
    specs += [dict(name="d_coef", nbytes=n * ch * plane, align=16, role="out", guard=ch * plane, row=4 * bs, rows_per_stream=ch * nb),
              word("d_wc", n * nb, "out", rps=nb), word("d_bits", n * nb, "out", rps=nb)]
    a = gb.build(_dev(), specs)
    a.load("d_file", np.array(files, np.int32)); a.load("d_first", np.array(first, np.int32))
    if count is not None:
        a.load("d_count", np.array(count, np.int32))
    p = a.ptr
    if ragged:
        a.load("d_payload", lay["payload"]); a.load("d_payloadOffs", lay["poffs"]); a.load("d_index", lay["index"]); a.load("d_indexOffs", lay["ioffs"])
        a.load("d_indexBlocks", lay["blocks"])
        dec.decode_crops_spectra_ragged_dev(len(lay["blocks"]), p("d_payload"), lay["payload"].size, p("d_payloadOffs"), p("d_index"), lay["index"].size,
                                            p("d_indexOffs"), p("d_indexBlocks"), n, p("d_file"), p("d_first"), p("d_count") if count is not None else 0,
                                            nb, flags, p("d_coef"), p("d_wc"), p("d_bits"))
    else:
        a.load("d_payload", lay["host"]); a.load("d_payloadBytes", lay["nbytes"]); a.load("d_index", lay["index"]); a.load("d_indexBlocks", lay["count"])
        dec.decode_crops_spectra_dev(lay["host"].shape[0], p("d_payload"), lay["host"].shape[1], p("d_payloadBytes"), p("d_index"), lay["index"].shape[1],
                                     p("d_indexBlocks"), n, p("d_file"), p("d_first"), p("d_count") if count is not None else 0,
                                     nb, flags, p("d_coef"), p("d_wc"), p("d_bits"))
    torch.cuda.synchronize()
    a.check()
    return (a.fetch("d_coef", np.float32).reshape(n, ch, nb, bs), a.fetch("d_wc", np.int32).reshape(n, nb), a.fetch("d_bits", np.int32).reshape(n, nb))


def crop_bits(dec, lay, ch, bs, files, first, nb, count=None):
    """d_bits of ulcx_decode_crops_dev for the same rows."""
    import torch
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(_dev())
    n = len(files)
    pay, nbytes, idx, cnt = t(lay["host"]), t(lay["nbytes"]), t(lay["index"].view(np.int32).reshape(lay["index"].shape[0], -1)), t(lay["count"])
    d_file, d_first = t(np.array(files, np.int32)), t(np.array(first, np.int32))
    d_count = t(np.array(count, np.int32)) if count is not None else None
    pcm = torch.full((n, nb, bs, ch), 7.0, dtype=torch.float32, device=_dev())
    bits = torch.full((n, nb), 7, dtype=torch.int32, device=_dev())
    dec.decode_crops_dev(lay["host"].shape[0], pay.data_ptr(), lay["host"].shape[1], nbytes.data_ptr(), idx.data_ptr(), lay["index"].shape[1], cnt.data_ptr(),
                         n, d_file.data_ptr(), d_first.data_ptr(), d_count.data_ptr() if d_count is not None else 0, nb, pcm.data_ptr(), bits.data_ptr())
    torch.cuda.synchronize()
    return bits.cpu().numpy()


def check(got, want, files, first, what):
    """coef, wc and bits of every row against the expected ones, bit for bit; the first row that differs is named."""
    for i in range(len(files)):
        where = f"{what}: row {i} (file {files[i]} from block {first[i]})"
        assert np.array_equal(got[2][i], want[2][i]), f"{where}: bits {got[2][i]} vs the oracle's {want[2][i]}"
        assert np.array_equal(got[1][i], want[1][i]), f"{where}: window codes {got[1][i]} vs {want[1][i]}"
        for c in range(want[0].shape[1]):
            for k in range(want[0].shape[2]):
                assert S.same_bits(got[0][i, c, k], want[0][i, c, k]), \
                    f"{where}: channel {c} of block {first[i] + k} differs at {np.flatnonzero(got[0][i, c, k].view(np.uint32) != want[0][i, c, k].view(np.uint32))[:4]}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. rows and counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_count", [False, True], ids=["no-count", "count"])
@pytest.mark.parametrize("geom", GEOMS)
def test_rows_equal_the_oracles_coefficients(geom, with_count):
    """70 rows in one call (more than a wave of the walk): first 0, first 1, starts directly behind window-switched blocks, rows that
    run past the file's end, first = the block count, many rows per file; counts of 0, 1, nBlocks and nBlocks + 3 in turn."""
    amd = _amd()
    bs, ch = geom
    cor = S.geom_corpus(geom)
    rows = S.seventy_rows(cor)
    files, first = [f for f, _ in rows], [k for _, k in rows]
    count = [(0, 1, N, N + 3)[i % 4] for i in range(len(rows))] if with_count else None
    dec = amd.BatchDecoder(len(rows), ch, bs, N + 1)
    got = spectra_dev(dec, cor.strided(), ch, bs, files, first, N, count)
    assert dec.last_cut()[:2] == (0, 0)                     # the plain plan: nothing of the synthesis's cuts applies
    want = cor.expected_spec(files, first, N, count)
    check(got, want, files, first, f"{bs} x {ch}")
    assert np.array_equal(got[2], crop_bits(dec, cor.strided(), ch, bs, files, first, N, count)), "d_bits differs from the crop call's"
    dec.close()
    live = want[2] > 0
    assert live.sum() >= (60 if with_count else 150) and (~live).sum() >= 20 and (want[0] != 0).any()
    assert ((want[1] != 0) == live).all() and len({int(w) for w in want[1].ravel()}) >= 4


# ---------------------------------------------------------------------------------------------------------------------
# 2. units of several noise passes
# ---------------------------------------------------------------------------------------------------------------------
def test_units_of_more_than_2048_noise_coefficients():
    amd = _amd()
    cor = S.geom_corpus((4096, 2))
    rows = S.noise_pass_rows()
    files, first = [f for f, _ in rows], [k for _, k in rows]
    dec = amd.BatchDecoder(len(rows), 2, 4096, N + 1)
    for flags in (0, LR):
        got = spectra_dev(dec, cor.strided(), 2, 4096, files, first, N, flags=flags)
        check(got, cor.expected_spec(files, first, N, lr=bool(flags)), files, first, f"4096 x 2, flags {flags}")
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. the LDS ceiling: one unit array per workgroup, and LR formed in place
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2])
def test_blocksize_32768_takes_the_one_array_path(ch):
    """32768 x 1: a decimated file (units of up to 15 996 noise coefficients) and a steady one whose last block is ONE unit of 32768
    with coded and noise coefficients; LR on mono is flags 0.  32768 x 2: two unit arrays do not fit a CU, so the pair goes through
    one array channel after channel and LR is formed in place on the plane the workgroup stored itself."""
    amd = _amd()
    cor = S.Corpus([S.big_stream(ch, True), S.big_stream(ch, False)] if ch == 1 else [S.big_stream(ch, True)])
    rows = [(f, k) for f in range(cor.F) for k in (0, 1)]
    files, first = [f for f, _ in rows], [k for _, k in rows]
    dec = amd.BatchDecoder(len(rows), ch, 32768, 3)
    plain = spectra_dev(dec, cor.strided(), ch, 32768, files, first, 2)
    check(plain, cor.expected_spec(files, first, 2), files, first, f"32768 x {ch}")
    lr = spectra_dev(dec, cor.strided(), ch, 32768, files, first, 2, flags=LR)
    check(lr, cor.expected_spec(files, first, 2, lr=True), files, first, f"32768 x {ch}, LR")
    if ch == 1:
        assert S.same_bits(lr[0], plain[0])
    else:
        assert not S.same_bits(lr[0][:, 0], plain[0][:, 0]) and not S.same_bits(lr[0][:, 1], plain[0][:, 1])
    assert np.array_equal(plain[2], crop_bits(dec, cor.strided(), ch, 32768, files, first, 2))
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. LR pairing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(2048, 2), (2048, 3), (1024, 6)])
def test_lr_unmixes_the_pairs_and_leaves_a_single_channel(geom):
    amd = _amd()
    bs, ch = geom
    cor = S.geom_corpus(geom)
    rows = S.row_table(cor)
    files, first = [f for f, _ in rows], [k for _, k in rows]
    dec = amd.BatchDecoder(len(rows), ch, bs, N + 1)
    got = spectra_dev(dec, cor.strided(), ch, bs, files, first, N, flags=LR)
    ms = cor.expected_spec(files, first, N)
    want = cor.expected_spec(files, first, N, lr=True)
    check(got, want, files, first, f"{bs} x {ch}, LR")
    dec.close()
    for c in range(0, ch - 1, 2):                           # the pairs (0,1), (2,3), ...: really un-mixed, in float32
        assert S.same_bits(got[0][:, c], ms[0][:, c] + ms[0][:, c + 1]) and S.same_bits(got[0][:, c + 1], ms[0][:, c] - ms[0][:, c + 1])
        assert not S.same_bits(got[0][:, c], ms[0][:, c])
    if ch & 1:
        assert S.same_bits(got[0][:, ch - 1], ms[0][:, ch - 1]) and (ms[0][:, ch - 1] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ragged layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LR], ids=["ms", "lr"])
def test_ragged_entries_equal_the_strided_ones(flags):
    """The 2048 x 2 corpus with its files back to back, and a third file - the first one's bytes again - whose payload offsets fall:
    its rows are zeros, the others are what the strided layout gives."""
    amd = _amd()
    cor = S.geom_corpus((2048, 2))
    three = S.Corpus(cor.files + [cor.files[0]])
    rg = three.ragged()
    rg["poffs"][3] = rg["poffs"][2] - 1                     # file 2 is bytes [poffs[2], poffs[2] - 1)
    rows = S.row_table(cor) + [(2, 0), (2, 7), (0, 9), (1, 3)]
    files, first = [f for f, _ in rows], [k for _, k in rows]
    count = [(N, N + 3, 1, N)[i % 4] for i in range(len(rows))]
    dec = amd.BatchDecoder(len(rows), 2, 2048, N + 1)
    got = spectra_dev(dec, rg, 2, 2048, files, first, N, count, flags)
    seen = [-1 if f == 2 else f for f in files]             # (a file number outside the corpus: the expected row is zeros)
    want = cor.expected_spec(seen, first, N, count, lr=bool(flags))
    check(got, want, files, first, "ragged")
    bad = [i for i, f in enumerate(files) if f == 2]
    assert len(bad) == 2 and not got[0][bad].any() and not got[1][bad].any() and not got[2][bad].any()
    ok = [i for i, f in enumerate(files) if f != 2]
    st = spectra_dev(dec, cor.strided(), 2, 2048, [files[i] for i in ok], [first[i] for i in ok], N, [count[i] for i in ok], flags)
    for j, i in enumerate(ok):
        assert S.same_bits(st[0][j], got[0][i]) and np.array_equal(st[1][j], got[1][i]) and np.array_equal(st[2][j], got[2][i]), i
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. host forms, refusals with an object
# ---------------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms_and_refuse_what_the_crop_host_forms_refuse():
    amd = _amd()
    cor = S.geom_corpus((2048, 3))
    rows = S.row_table(cor)
    files, first = [f for f, _ in rows], [k for _, k in rows]
    count = [(N, 2, N + 3, 0)[i % 4] for i in range(len(rows))]
    dec = amd.BatchDecoder(len(rows), 3, 2048, N + 1)
    rg = cor.ragged()
    for flags in (0, LR):
        want = cor.expected_spec(files, first, N, count, lr=bool(flags))
        dev = spectra_dev(dec, cor.strided(), 3, 2048, files, first, N, count, flags)
        check(dev, want, files, first, "device form")
        host = dec.decode_crops_spectra(cor.host, cor.nbytes, cor.index, cor.count, files, first, N, count=count, flags=flags)
        check(host, want, files, first, "host form")
        hr = dec.decode_crops_spectra_ragged(rg["payload"], rg["poffs"], rg["index"], rg["ioffs"], rg["blocks"], files, first, N, count=count, flags=flags)
        check(hr, want, files, first, "ragged host form")
    # what ulcx_decode_crops_host / _ragged_host refuse, before any device work: a file out of range, a first outside [0, blocks], a
    # negative count; the ragged form also an offset table that falls.  And every form an unknown flag bit.
    K = cor.K[0]
    for hf, h1, hc, why in (([0, 1], [0, 0], None, "names file 1"), ([0, -1], [0, 0], None, "names file -1"), ([0, 0], [0, K + 1], None, "starts at block"),
                            ([0, 0], [0, -1], None, "starts at block"), ([0, 0], [0, 0], [1, -1], "wants -1 blocks")):
        with pytest.raises(amd.UlcError, match=why):
            dec.decode_crops_spectra(cor.host, cor.nbytes, cor.index, cor.count, hf, h1, N, count=hc)
        with pytest.raises(amd.UlcError, match=why):
            dec.decode_crops_spectra_ragged(rg["payload"], rg["poffs"], rg["index"], rg["ioffs"], rg["blocks"], hf, h1, N, count=hc)
    falls = rg["poffs"].copy(); falls[1] = -4
    with pytest.raises(amd.UlcError, match="payload buffer"):
        dec.decode_crops_spectra_ragged(rg["payload"], falls, rg["index"], rg["ioffs"], rg["blocks"], [0], [0], N)
    with pytest.raises(amd.UlcError, match="flags"):
        dec.decode_crops_spectra(cor.host, cor.nbytes, cor.index, cor.count, [0], [0], N, flags=2)
    with pytest.raises(amd.UlcError, match="nBlocks"):
        dec.decode_crops_spectra(cor.host, cor.nbytes, cor.index, cor.count, [0], [0], N + 1)
    dec.close()


def test_misaligned_outputs_and_too_many_rows_are_refused_before_any_device_work():
    import torch
    amd = _amd()
    cor = S.geom_corpus((2048, 2))
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(_dev())
    pay, nbytes, idx, cnt = t(cor.host), t(cor.nbytes), t(cor.index.view(np.int32).reshape(cor.F, -1)), t(cor.count)
    d_file, d_first = t(np.array([0, 1, 0], np.int32)), t(np.array([3, 0, 9], np.int32))
    coef = torch.full((2 * 2 * N * 2048 + 8,), 7.0, dtype=torch.float32, device=_dev())
    wc = torch.full((2 * N + 2,), 7, dtype=torch.int32, device=_dev())
    bits = torch.full((2 * N + 2,), 7, dtype=torch.int32, device=_dev())
    dec = amd.BatchDecoder(2, 2, 2048, N + 1)

    def call(n=2, co=0, wo=0, bo=0, flags=0):
        dec.decode_crops_spectra_dev(cor.F, pay.data_ptr(), cor.stride, nbytes.data_ptr(), idx.data_ptr(), cor.istride, cnt.data_ptr(), n, d_file.data_ptr(),
                                     d_first.data_ptr(), 0, N, flags, coef.data_ptr() + co, wc.data_ptr() + wo, bits.data_ptr() + bo)
    for kw, name in ((dict(co=4), "d_coef"), (dict(co=8), "d_coef"), (dict(wo=2), "d_wc"), (dict(bo=1), "d_bits")):
        with pytest.raises(amd.UlcError, match=r"\(-1\).*" + name + r".*not aligned"):
            call(**kw)
    with pytest.raises(amd.UlcError, match=r"\(-1\).*flags"):
        call(flags=LR | 4)
    with pytest.raises(amd.UlcError, match=r"\(-1\).*n 3"):
        call(n=3)
    torch.cuda.synchronize()
    assert (coef == 7.0).all() and (wc == 7).all() and (bits == 7).all(), "a refused call wrote"
    call()
    torch.cuda.synchronize()
    want = cor.expected_spec([0, 1], [3, 0], N)
    got = (coef[:2 * 2 * N * 2048].cpu().numpy().reshape(2, 2, N, 2048), wc[:2 * N].cpu().numpy().reshape(2, N), bits[:2 * N].cpu().numpy().reshape(2, N))
    check(got, want, [0, 1], [3, 0], "valid call behind the refused ones")
    assert (coef[2 * 2 * N * 2048:] == 7.0).all() and (wc[2 * N:] == 7).all() and (bits[2 * N:] == 7).all()
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the object's state
# ---------------------------------------------------------------------------------------------------------------------
def test_a_streaming_decode_continues_across_spectra_calls_and_a_sample_crop_behind_one_is_unaffected():
    import torch
    amd = _amd()
    cor = S.geom_corpus((2048, 2))
    bs, ch, B, K = 2048, 2, 4, 4
    srcs = [cor.files[s % 2] for s in range(B)]
    slot = max(f.blocks.shape[1] for f in srcs)
    blocks = np.zeros((B, 3 * K, slot), np.uint8)
    for s, f in enumerate(srcs):
        blocks[s, :, :f.blocks.shape[1]] = f.blocks[:3 * K]
    refs = [oracle_pcm(f.blocks, ch, bs) for f in srcs]
    dec = amd.BatchDecoder(B, ch, bs, max(K, N + 1))
    d_in = torch.from_numpy(blocks).to(_dev())
    rows = S.row_table(cor)[:B]
    files, first = [f for f, _ in rows], [k for _, k in rows]

    def stream_call(j):
        pcm = torch.full((B, K, bs, ch), 7.0, dtype=torch.float32, device=_dev())
        bits = torch.full((B, K), 7, dtype=torch.int32, device=_dev())
        part = d_in[:, j * K:(j + 1) * K].contiguous()
        dec.decode_dev(part.data_ptr(), slot, K, pcm.data_ptr(), bits.data_ptr())
        torch.cuda.synchronize()
        for s in range(B):
            assert np.array_equal(bits[s].cpu().numpy(), refs[s][1][j * K:(j + 1) * K]), (j, s)
            assert S.same_bits(pcm[s].cpu().numpy(), refs[s][0][j * K:(j + 1) * K]), f"streaming call {j}, stream {s}"

    stream_call(0)
    before = dec.save_streams(list(range(B)))
    for flags in (0, LR):
        got = spectra_dev(dec, cor.strided(), ch, bs, files, first, N, flags=flags)
        check(got, cor.expected_spec(files, first, N, lr=bool(flags)), files, first, "between two streaming calls")
    assert before.tobytes() == dec.save_streams(list(range(B))).tobytes(), "a spectra call changed a stream's state"
    stream_call(1)
    # a sample-crop call behind a spectra call: the oracle's samples, channels-first
    spectra_dev(dec, cor.strided(), ch, bs, files, first, N)
    start, ns = [3 * bs + 100, 0, 20 * bs - 7], 2 * bs + 13
    pcm, _ = dec.decode_crops_samples(cor.host, cor.nbytes, cor.index, cor.count, [0, 1, 0], start, ns)
    for i, (f, st) in enumerate(zip([0, 1, 0], start)):
        flat = oracle_pcm(cor.files[f].blocks, ch, bs)[0].reshape(-1, ch)
        assert S.same_bits(pcm[i], flat[st:st + ns].T), f"sample crop row {i} behind a spectra call"
    stream_call(2)
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. damaged payloads under a stored index
# ---------------------------------------------------------------------------------------------------------------------
def test_damaged_blocks_end_rows_and_displace_the_noise_as_in_the_crop_call():
    """2048 x 2, block 7 of a file damaged behind its index: killed (a row with it in the middle ends there; a row with it in front is
    all zeros), and value-damaged so that it still parses (the row lives, and where the damage changes the block's draws the noise
    of the blocks behind it follows the draws actually made).  Expected: the oracle run block by block from the stored generator
    state (spectra_testlib.damaged_row, damage_testlib's model with coefficients for samples).  d_bits is the crop call's."""
    amd = _amd()
    st = D.stream_of((2048, 2))
    j = 7
    dc = D.DamagedCorpus(st, [("kill", j), ("value", j), ("draws", j)])
    kill, val = dc.of_kind("kill", j)[0], dc.of_kind("value", j)[0]
    rows = [(0, j - 2), (kill, j - 2), (kill, j + 1), (kill, j), (kill, j + 2), (val, j - 2), (val, j + 1), (val, j - N)]
    for f in dc.of_kind("draws", j):
        rows += [(f, j - 2), (f, j + 1)]
    files, first = [f for f, _ in rows], [k for _, k in rows]
    want = [np.zeros((len(rows), 2, N, 2048), np.float32), np.zeros((len(rows), N), np.int32), np.zeros((len(rows), N), np.int32)]
    live = []
    for i, (f, k) in enumerate(rows):
        want[0][i], want[1][i], want[2][i], lv = S.damaged_row(dc.payloads[f], st.offs, st.seeds, 2, 2048, k, N)
        live.append(lv)
    assert live[:5] == [N, 2, 0, 0, N] and live[5:8] == [N, N, N], live          # dead in the middle, dead in front, dead first, clean behind it
    clean = S.damaged_row(dc.payloads[0], st.offs, st.seeds, 2, 2048, j - 2, N)[0]
    assert S.same_bits(want[0][0], clean) and not S.same_bits(want[0][5][:, 2], clean[:, 2]) and S.same_bits(want[0][5][:, :2], clean[:, :2])
    for i in range(8, len(rows), 2):                        # a damage that moves the generator: the noise of the blocks behind it differs
        assert not S.same_bits(want[0][i][:, 3:], clean[:, 3:])
    lay = dict(host=dc.host, nbytes=dc.nbytes, index=dc.index, count=dc.count)
    dec = amd.BatchDecoder(len(rows), 2, 2048, N + 1)
    got = spectra_dev(dec, lay, 2, 2048, files, first, N)
    check(got, want, files, first, "damaged")
    assert np.array_equal(got[2], crop_bits(dec, lay, 2, 2048, files, first, N)), "d_bits differs from the crop call's"
    dec.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. corpus.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["strided", "ragged"])
def test_crop_corpus_spectra_is_the_c_call(layout):
    import struct
    import torch
    import corpus
    amd = _amd()
    cor = S.geom_corpus((2048, 2))
    cc = corpus.CropCorpus(cor.ch, cor.bs, layout=layout)
    for f in range(cor.F):
        pay = cor.host[f, :cor.nbytes[f]].tobytes()
        ulc = struct.pack("<IHHIIHHI", 0x32434C55, cor.bs, 0, cor.K[f], 44100, cor.ch, 0, 24) + pay
        assert cc.add_file(ulc, amd.ulx_pack(cor.index[f], cor.K[f], cor.bs, cor.ch, len(pay)) if f == 0 else None) == f
    cc.freeze("cuda:0")
    rows = S.row_table(cor)
    files, first = [f for f, _ in rows], [k for _, k in rows]
    count = [(N, 3, N + 3, 0)[i % 4] for i in range(len(rows))]
    dec = amd.BatchDecoder(len(rows), cor.ch, cor.bs, N + 1)
    for lr in (False, True):
        coef, wc, bits = cc.spectra(dec, files, torch.tensor(first, dtype=torch.int32, device="cuda:0"), N, count=count, lr=lr)
        assert tuple(coef.shape) == (len(rows), cor.ch, N, cor.bs) and coef.is_cuda and coef.dtype == torch.float32
        assert tuple(wc.shape) == tuple(bits.shape) == (len(rows), N) and wc.dtype == bits.dtype == torch.int32
        torch.cuda.synchronize()
        got = (coef.cpu().numpy(), wc.cpu().numpy(), bits.cpu().numpy())
        check(got, cor.expected_spec(files, first, N, count, lr=lr), files, first, f"CropCorpus.spectra, {layout}")
        c_call = spectra_dev(dec, cor.strided(), cor.ch, cor.bs, files, first, N, count, LR if lr else 0)
        assert S.same_bits(got[0], c_call[0]) and np.array_equal(got[1], c_call[1]) and np.array_equal(got[2], c_call[2])
    dec.close()
